// ransac_device.h -- every device header of the RANSAC minimal solvers, for the translation units that want them all
// (ransac.hip, selftest_team_solvers.hip).  Includes only: anything else names the headers it uses.
#pragma once
#include "small_linalg.h"
#include "eig_general.h"
#include "rotation_maps.h"
#include "sqpnp_device.h"
#include "five_point_device.h"
#include "twoview_device.h"
#include "position_plane_device.h"
#include "p3p_device.h"
#include "radial_homography_device.h"
