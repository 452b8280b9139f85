"""The geometry either side of the solve on the device against the mpmath model of tests/geometry_reference.py, which shares
nothing with the kernels or the CPU oracle: the filter (kernels_filter.hip: reproject, validate), track creation
(kernels_tracks.hip: rays through the fixed-point undistortion, the cofactor triangulation and its four tests), the RS-PnP
scoring rule with its float32 roundings and one trust-region step of the hypothesis kernel (kernels_pnp.hip).  The checks, their
constants and the margin rules that say which items rounding may decide are those of tests/test_geometry_reference.py, where the
CPU oracle goes through the same functions; flags are exact on decided items, and every test prints its largest ratio and its
undecided count.

Measured (device on an MI355X | CPU oracle), in the units of each bound:
  A  reproject, pixels in 2^-53 (|xy| + fx + fy) amp (C_A = 128): 12.0 | 11.4 (both: the clamped items of the frame whose poses
     are 20 apart, projected 7000 - 18000 px outside the image, where the distortion polynomial multiplies the rounding of
     the normalised point; 1.43 | 1.43 inside it); no item undecided of 3 511
  B  validate: every flag equal, the 64-observation band at threshold (1 +- 2^-20) included; no item undecided
  C  tri_pt in cond(A) 2^-53 (|c1| + |c2| + |p|) amp_u (C_C = 32): 2.84 | 2.84 (triangulate alone on exact rays 0.89), down
     to det(A) = 1.4e-9, cond(A) = 5.9e9; no flag undecided of 1 369 candidates; 17 of 32 exactly parallel pairs solved
  D  scoring: every decided flag equal; 1 of 16 575 (hypothesis, point) pairs undecided
  E  one LM step in kappa 2^-53 |delta|_inf (C_TOL = 64, kappa 59 - 5.2e4): 3.1 | 2.4; final cost over the start cost
     (C_E = 3.3e-13): 1.6e-14 | 2.0e-14 (VERTICAL, m = 6: the functor's tau from x fits poorly there and leaves a cost of 30)."""
import numpy as np
import pytest

import geometry_reference as G
import test_geometry_reference as T
from rsba_amd.problem import BAProblem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from rsba_amd import capi
    assert capi.device_count() >= 1
    return capi


@pytest.fixture(scope="module")
def tracks():
    return {key: G.tracks_model(G.tracks_case(*key), T.C_C)[0] for key in G.C_CASES}


# ---- A ----
@pytest.mark.parametrize("key", G.A_HANDLE, ids=str)
def test_reproject_of_a_session(capi, key):
    case, model = G.reproject_handle_case(*key), G.reproject_model(G.reproject_handle_case, *key)
    with capi.DeviceProblem(BAProblem(**case["prob"])) as dp:
        xy, ok = dp.reproject(case["frames"], case["points"])
    worst, undecided = T.check_reproject(case, model, xy, ok)
    print(f"reproject {key}: worst {worst:.2f}, undecided {undecided} of {len(model)}")


@pytest.mark.parametrize("key", G.A_FRAME, ids=str)
def test_reproject_of_one_frame(capi, key):
    case, model = G.reproject_frame_case(*key), G.reproject_model(G.reproject_frame_case, *key)
    xy, ok = capi.reproject_frame(case["cam"], case["poses"], case["shutter"], case["scan"], case["X"], case["interp"])
    worst, undecided = T.check_reproject(case, model, xy, ok)
    print(f"reproject_frame {key}: worst {worst:.2f}, undecided {undecided} of {len(model)}")


# ---- B ----
@pytest.mark.parametrize("key", G.B_HANDLE, ids=str)
def test_validate_of_a_session(capi, key):
    case, model = G.validate_handle_case(*key), G.validate_model(G.validate_handle_case, *key)
    with capi.DeviceProblem(BAProblem(**case["prob"])) as dp:
        flags = dp.validate_observations(case["thr"], case["min_dist"])
    print(f"validate {key}: undecided {T.check_validate(case, model, flags)} of {len(model)}")


@pytest.mark.parametrize("key", G.B_FRAME, ids=str)
def test_validate_of_a_scan_line_frame(capi, key):
    case, model = G.validate_frame_case(*key), G.validate_model(G.validate_frame_case, *key)
    flags = capi.validate_frame(case["cam"], case["poses"], case["shutter"], case["scan"], case["X"], case["xy"], case["thr"], case["min_dist"])
    print(f"validate_frame {key}: undecided {T.check_validate(case, model, flags)} of {len(model)}")


# ---- C ----
def device_tracks(capi, case):
    return capi.track_candidates(case["cams"], case["fcam"], case["fposes"], case["shutter"], case["scan"], case["of"], case["oxy"], case["ca"], case["cb"],
                                 case["request"], case["track_pt"], case["thr"], case["min_dist"], case["interp"])


@pytest.mark.parametrize("key", G.C_CASES, ids=str)
def test_track_candidates(capi, tracks, key):
    case = G.tracks_case(*key)
    worst, undecided = T.check_tracks(case, tracks[key], *device_tracks(capi, case))
    print(f"track_candidates {key}: worst {worst:.2f}, undecided {undecided} of {len(tracks[key])}")


def test_parallel_rays_write_no_point_unless_solved(capi):
    """det(A) is about 0: whether the solve runs is rounding's choice, but a point is written only if it did and accepted only then"""
    case = G.parallel_case()
    tri_ok, tri_pt, rep_ok = device_tracks(capi, case)
    written = np.any(tri_pt != 0, axis=1)
    assert np.all(np.isfinite(tri_pt)) and not tri_ok[~written].any() and not rep_ok.any()
    print(f"parallel rays: {int(written.sum())} of {len(written)} solved")


# ---- D ----
@pytest.mark.parametrize("key", G.D_CASES, ids=str)
def test_scores_of_given_poses(capi, key):
    case, model = G.score_case(*key), G.score_model(*key)
    out = capi.pnp_tasks(G.CAM, case["shutter"], case["scan"], case["X"], case["xy"], case["subs"], case["inits"], max_num_iterations=0,
                         reprojection_error=case["thr"])
    assert np.all(out["status"] == 1) and np.array_equal(out["poses"].reshape(-1, 12), case["inits"])
    mask = capi.pnp_inliers(G.CAM, case["shutter"], case["scan"], case["X"], case["xy"], case["inits"][0], case["thr"])
    undecided = T.check_scores(case, model, out["num_inliers"], mask)
    print(f"pnp scoring {key}: undecided {undecided} of {len(model) * len(model[0])}")


# ---- E ----
@pytest.mark.parametrize("key", T.E_KEYS, ids=str)
def test_first_step_of_the_hypothesis_kernel(capi, key):
    call, model = G.step_call(*key), G.step_model(*key)
    out = capi.pnp_tasks(G.CAM, call["shutter"], call["scan"], call["X"], call["xy"], call["subs"], call["inits"] if call["per_task"] else call["inits"][0],
                         max_num_iterations=1, reprojection_error=8.0)
    assert np.all(out["status"] == 1)
    worst, worst_cost = T.check_steps(call, model, out["poses"], out["final_cost"])
    print(f"LM step {key}: worst {worst:.3f} of kappa eps |delta|, cost {worst_cost:.1e} of cost0")
