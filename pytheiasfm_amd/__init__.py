"""pytheiasfm_amd -- MI355X-native bundle adjustment + RANSAC engine behind
pyTheia's BundleAdjust* / Estimate* entry points."""
__version__ = "0.1.0"

from . import camera  # noqa: E402,F401
from . import incremental  # noqa: E402,F401
from .incremental import (FindViewsToLocalize, VisibilityPyramid, LocalizeViewToReconstruction,  # noqa: E402,F401
                          LocalizeViewsToReconstruction, LocalizeViewToReconstructionOptions,
                          SetUnderconstrainedAsUnestimated, SetUnderconstrainedTracksToUnestimated,
                          SetUnderconstrainedViewsToUnestimated, NumEstimatedViews, NumEstimatedTracks,
                          OrderViewPairsByInitializationCriterion)
from . import alignment  # noqa: E402,F401
from .alignment import (AlignPointCloudsUmeyama, AlignPointCloudsUmeyamaWithWeights,  # noqa: E402,F401
                        AlignPointCloudsUmeyamaBatch, AlignPointCloudsUmeyamaWithWeightsBatch, AlignReconstructions,
                        AlignReconstructionsRobust, TransformReconstruction, TransformReconstruction4,
                        FindCommonViewsByName, AlignRotations, AlignOrientations,
                        Sim3AlignmentType, Sim3AlignmentOptions, Sim3AlignmentSummary, OptimizeAlignmentSim3,
                        OptimizeAlignmentSim3Batch, Sim3FromRotationTranslationScale, Sim3ToRotationTranslationScale,
                        Sim3ToHomogeneousMatrix, Sim3PoseGraphOptions, Sim3PoseGraphSummary, OptimizePoseGraphSim3,
                        Sim3sFromReconstruction, RelativeSim3s, SetPosesFromSim3s, AlignOverlapReconstructionsPoseGraph)
