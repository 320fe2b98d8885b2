"""CPU-only: the camera-path helpers of mvsnerf_amd.utils against the reference's own outputs (tests/golden/caseE_paths.npz, written by
tests/gen_golden_paths.py from the reference's functions).  The same numpy / scipy calls in the same order give the same bits: np.array_equal."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import gen_golden_paths as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "caseE_paths.npz"))
    return {k: z[k] for k in z.files}


def _same(got, want):
    got = got.numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())


def test_golden_inputs_are_the_generators(gold):
    for k, v in G.inputs().items():
        assert v.tobytes() == gold[k].tobytes(), k


@pytest.mark.parametrize("n,n_views", G.PATH_CASES)
def test_gen_render_path(gold, n, n_views):
    from mvsnerf_amd import utils
    want = gold[f"path{n}_views{n_views}"]
    assert want.shape == (n * (n_views // 3), 4, 4) and want.dtype == np.float64
    _same(utils.gen_render_path(gold[f"path{n}_c2ws"], N_views=n_views), want)


def test_gen_render_path_default_and_unwrap(gold):
    from mvsnerf_amd import utils
    _same(utils.gen_render_path(gold["path3_c2ws"]), gold["path3_default"])
    assert gold["path3_default"].shape == (30, 4, 4)
    _same(utils.gen_render_path(gold["cross_c2ws"], N_views=12), gold["cross_views12"])


def test_gen_render_path_spherical(gold):
    from mvsnerf_amd import utils
    for k, (theta, phi, radius) in enumerate(gold["spherical_args"]):
        got = utils.gen_render_path_spherical(float(theta), float(phi), float(radius))
        assert torch.is_tensor(got) and got.dtype == torch.float32
        _same(got, gold[f"spherical{k}"])
    _same(utils.gen_render_path_spherical(30.0, -30.0), gold["spherical_default"])


def test_pose_spherical_nerf_and_normalize(gold):
    from mvsnerf_amd import utils
    for k, e in enumerate(gold["nerf_euler"]):
        _same(utils.pose_spherical_nerf(e), gold[f"nerf{k}"])
    _same(utils.pose_spherical_nerf(gold["nerf_euler"][1], radius=2.0), gold["nerf_radius2"])
    _same(utils.normalize(gold["normalize_v"]), gold["normalize_out"])


def test_pose_spherical_dtu(gold):
    from mvsnerf_amd import utils
    assert gold["dtu8"].shape == (8, 3, 4)
    _same(utils.pose_spherical_dtu(gold["dtu_radii"], float(gold["dtu_focus"].reshape(-1)[0]), n_poses=8), gold["dtu8"])
    _same(utils.pose_spherical_dtu(gold["dtu_radii"], float(gold["dtu_focus"].reshape(-1)[0]), n_poses=8, world_center=gold["dtu_center"]), gold["dtu8_center"])


@pytest.mark.parametrize("k", [1, 3])
def test_get_nearest_pose_ids(gold, k):
    from mvsnerf_amd import utils
    assert gold[f"nearest{k}"].shape == (4, k)
    _same(utils.get_nearest_pose_ids(gold["nearest_tar"], gold["nearest_ref"], k), gold[f"nearest{k}"])


def test_signatures_are_the_references():
    from mvsnerf_amd import utils
    P, K = inspect.Parameter, inspect.Parameter.POSITIONAL_OR_KEYWORD
    sig = lambda *ps: inspect.Signature(list(ps))
    assert inspect.signature(utils.gen_render_path) == sig(P("c2ws", K), P("N_views", K, default=30))
    assert inspect.signature(utils.gen_render_path_spherical) == sig(P("theta", K), P("phi", K), P("radius", K, default=1.0))
    assert inspect.signature(utils.pose_spherical_nerf) == sig(P("euler", K), P("radius", K, default=4.0))
    assert inspect.signature(utils.normalize) == sig(P("v", K))
    assert inspect.signature(utils.get_nearest_pose_ids) == sig(P("tar_pose", K), P("ref_poses", K), P("num_select", K))
    s = inspect.signature(utils.pose_spherical_dtu)
    assert list(s.parameters) == ["radii", "focus_depth", "n_poses", "world_center"]
    assert all(p.kind == K for p in s.parameters.values())
    assert s.parameters["radii"].default is P.empty and s.parameters["focus_depth"].default is P.empty and s.parameters["n_poses"].default == 120
    wc = s.parameters["world_center"].default
    assert isinstance(wc, np.ndarray) and wc.dtype == np.array([0, 0, 0]).dtype and wc.tolist() == [0, 0, 0]
    # the depth colour maps: the reference's names and order; cmap is a table here (cv2's colour-map number there)
    for fn in (utils.visualize_depth_numpy, utils.visualize_depth):
        assert inspect.signature(fn) == sig(P("depth", K), P("minmax", K, default=None), P("cmap", K, default=None))
    assert inspect.signature(utils.save_frames) == sig(P("frames", K), P("directory", K), P("prefix", K, default=""))


def test_star_import_offers_the_names_and_not_pixelnerf():
    from mvsnerf_amd import utils
    ns = {}
    exec("from mvsnerf_amd.utils import *", ns)
    for name in ("gen_render_path", "gen_render_path_spherical", "pose_spherical_nerf", "pose_spherical_dtu", "normalize", "get_nearest_pose_ids",
                 "visualize_depth", "visualize_depth_numpy", "save_frames"):
        assert name in ns, name
    # left out on purpose: the reference's own raises UnboundLocalError (it rebinds R before reading it, utils.py:565)
    assert not hasattr(utils, "gen_render_path_pixelNeRF") and not hasattr(utils, "get_scheduler")


def test_render_path_methods_exist():
    from mvsnerf_amd import train
    s = inspect.signature(train.MVSSystem.render_path)
    assert list(s.parameters) == ["self", "batch", "c2ws_render", "hw", "intrinsic", "near_far", "depth_panel", "crop", "minmax", "cmap", "volume"]
    assert [s.parameters[k].default for k in list(s.parameters)[3:]] == [None, None, None, True, False, None, None, None]
    for cls in (train.MVSSystemFinetune, train.MVSSystemFusion):
        assert list(inspect.signature(cls.render_path).parameters)[:4] == ["self", "c2ws_render", "hw", "focal"]
