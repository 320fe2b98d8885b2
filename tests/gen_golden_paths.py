"""Writes tests/golden/caseE_paths.npz from the reference's OWN camera-path helpers on the CPU (needs the reference checkout, see oracle/ref_shim.py):
gen_render_path, gen_render_path_spherical, pose_spherical_nerf, normalize, pose_spherical_dtu, get_nearest_pose_ids (utils.py:479-534, 634-676,
698-711) through oracle.ref_shim.load_reference(), on the seeded inputs below.

  * gen_render_path: three and five random c2ws whose 'xyz' Euler angles stay within +-40 degrees (the +-180 degree unwrap of :488-489 stays quiet), with
    N_views 3, 12, 30, and one case of three poses whose angles cross 180 degrees on purpose (the unwrap adds 360).
  * gen_render_path_spherical: four (theta, phi, radius) triples; pose_spherical_nerf: three Euler triples (and one radius other than the default).
  * pose_spherical_dtu with n_poses 8 (and a world centre); normalize on one vector.
  * get_nearest_pose_ids: 4 target x 6 reference poses, num_select 1 and 3, no ties in distance (asserted).

Only inputs and outputs are stored.      python tests/gen_golden_paths.py [--check]     (--check: regenerate and compare bit for bit)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "caseE_paths.npz")
PATH_CASES = [(3, 3), (3, 12), (3, 30), (5, 3), (5, 12), (5, 30)]          # (number of poses, N_views)
SPHERICAL = [(0.0, 0.0, 1.0), (30.0, -30.0, 4.0), (-135.0, 12.5, 2.5), (90.0, -89.0, 0.75)]      # theta, phi, radius
NERF_EULER = [(0.0, 0.0, 0.0), (10.0, -25.0, 40.0), (-170.0, 65.0, 120.0)]
CROSSING = [(170.0, 10.0, -20.0), (-175.0, 20.0, -10.0), (160.0, -30.0, 175.0)]                   # 'xyz' degrees: x and z are more than 180 from pose 0's


def poses_from_euler(euler_deg, positions):
    from scipy.spatial.transform import Rotation
    c2ws = np.tile(np.eye(4), (len(euler_deg), 1, 1))
    c2ws[:, :3, :3] = Rotation.from_euler("xyz", np.asarray(euler_deg, dtype=np.float64), degrees=True).as_matrix()
    c2ws[:, :3, 3] = positions
    return c2ws


def inputs():
    rng = np.random.default_rng(20)
    out = {}
    for n, _ in PATH_CASES:
        if f"path{n}_c2ws" not in out:
            out[f"path{n}_c2ws"] = poses_from_euler(rng.uniform(-40.0, 40.0, (n, 3)), rng.uniform(-1.0, 1.0, (n, 3)))
    out["cross_c2ws"] = poses_from_euler(CROSSING, rng.uniform(-1.0, 1.0, (3, 3)))
    from scipy.spatial.transform import Rotation
    e = Rotation.from_matrix(out["cross_c2ws"][:, :3, :3]).as_euler("xyz", degrees=True)
    assert (np.abs(e[1:] - e[:1]) > 180).any() and (np.abs(np.asarray(CROSSING)[:, 1]) < 90).all()      # the unwrap branch really runs
    out["spherical_args"] = np.asarray(SPHERICAL, dtype=np.float64)
    out["nerf_euler"] = np.asarray(NERF_EULER, dtype=np.float64)
    out["dtu_radii"] = np.array([0.6, 0.4, 0.2])
    out["dtu_focus"] = np.array(3.5)
    out["dtu_center"] = np.array([0.1, -0.2, 3.0])
    out["normalize_v"] = rng.normal(size=(3,))
    tar, ref = rng.normal(size=(4, 4, 4)), rng.normal(size=(6, 4, 4))
    d = np.sort(np.linalg.norm(tar[:, None, :3, 3] - ref[None, :, :3, 3], axis=-1), axis=-1)
    assert float(np.diff(d, axis=-1).min()) > 1e-3                           # no ties: the argsort is unambiguous
    out["nearest_tar"], out["nearest_ref"] = tar, ref
    return out


def generate():
    from oracle import ref_shim
    U = ref_shim.load_reference()[2]
    out = inputs()
    for n, nv in PATH_CASES:
        out[f"path{n}_views{nv}"] = U.gen_render_path(out[f"path{n}_c2ws"], N_views=nv)
    out["path3_default"] = U.gen_render_path(out["path3_c2ws"])
    out["cross_views12"] = U.gen_render_path(out["cross_c2ws"], N_views=12)
    for k, (theta, phi, radius) in enumerate(SPHERICAL):
        out[f"spherical{k}"] = U.gen_render_path_spherical(theta, phi, radius).numpy()
    out["spherical_default"] = U.gen_render_path_spherical(30.0, -30.0).numpy()
    for k, e in enumerate(NERF_EULER):
        out[f"nerf{k}"] = U.pose_spherical_nerf(np.asarray(e))
    out["nerf_radius2"] = U.pose_spherical_nerf(np.asarray(NERF_EULER[1]), radius=2.0)
    out["dtu8"] = U.pose_spherical_dtu(out["dtu_radii"], float(out["dtu_focus"]), n_poses=8)
    out["dtu8_center"] = U.pose_spherical_dtu(out["dtu_radii"], float(out["dtu_focus"]), n_poses=8, world_center=out["dtu_center"])
    out["normalize_out"] = U.normalize(out["normalize_v"])
    for k in (1, 3):
        out[f"nearest{k}"] = U.get_nearest_pose_ids(out["nearest_tar"], out["nearest_ref"], k)
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def check():
    new, old = generate(), np.load(OUT)
    assert sorted(new) == sorted(old.files), sorted(set(new) ^ set(old.files))
    for k, v in new.items():
        assert v.dtype == old[k].dtype and v.shape == old[k].shape and v.tobytes() == old[k].tobytes(), f"{k} differs from the committed golden"
    return len(new)


if __name__ == "__main__":
    if "--check" in sys.argv:
        print(f"caseE_paths.npz: {check()} arrays regenerate bit for bit")
    else:
        np.savez_compressed(OUT, **generate())
        print("wrote", OUT, os.path.getsize(OUT), "bytes")
