"""pt.mvs: ViewSelectionMVSNet (pybind mvs.cc:44), on the device (covisibility.py)."""
from .covisibility import ViewSelectionMVSNet  # noqa: F401
