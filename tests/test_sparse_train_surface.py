"""CPU-only: the surface of the fine-tuning step that skips empty space - the compact_rows symbol, its argument codes, and the refusals that come
before the library."""
import os
import re
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mvsnerf_compact_rows_fwd"
OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
PTR = 0x10000        # non-NULL, 16-byte aligned, never dereferenced


def test_symbol_is_declared_exported_and_bound():
    from mvsnerf_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip_internal.h")).read(), flags=re.S)
    stable = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvsnerf_hip.h")).read(), flags=re.S)
    assert re.search(rf"\b{NAME}\s*\(", hdr)
    assert not re.search(rf"\b{NAME}\s*\(", stable)                      # internal tier only: the stable header and its ABI number do not change
    assert NAME in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert NAME in {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert _lib.lib().mvsnerf_abi_version() == 12
    assert callable(ops.compact_rows) and callable(ops.raymarch_sparse_train) and issubclass(ops.SparseRayMarchFunction, torch.autograd.Function)


def test_entry_refuses_bad_arguments_before_any_launch():
    from mvsnerf_amd import _lib
    L = _lib.lib()

    def compact(src=PTR, idx=PTR, count=PTR, P=32, n=8, C=4, dst=PTR):
        return L.mvsnerf_compact_rows_fwd(src, idx, count, P, n, C, dst, None)
    for kw in (dict(count=0), dict(dst=0), dict(src=0), dict(idx=0), dict(P=-1), dict(n=-1), dict(C=0), dict(n=33)):
        assert compact(**kw) == EINVAL, kw
    assert compact(C=65) == EUNSUPPORTED and compact(n=0, P=2 ** 31) == EUNSUPPORTED
    assert compact(C=65, dst=PTR + 2) == EUNSUPPORTED                    # the order of mvsnerf_expand_rows_fwd: unsupported before misaligned
    assert compact(C=0, P=2 ** 31) == EINVAL                             # ... and invalid before unsupported
    assert compact(dst=PTR + 2) == EALIGN and compact(count=PTR + 1) == EALIGN and compact(src=PTR + 3) == EALIGN and compact(idx=PTR + 2) == EALIGN
    assert compact(n=0) == OK and compact(n=0, P=0, src=0, idx=0) == OK  # nothing to write, nothing launched
    assert compact(n=0, C=1) == OK


def test_python_faces_refuse_before_the_library(monkeypatch):
    from mvsnerf_amd import _lib, models, ops, train

    def boom():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "lib", boom)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.compact_rows(torch.zeros((4, 4), requires_grad=True), i32(4), i32(1), 2)
    with pytest.raises(RuntimeError, match=r"\(P,C\)"):
        ops.compact_rows(torch.zeros((4, 4, 1)), i32(4), i32(1), 2)
    with pytest.raises(RuntimeError, match="int32 device tensors"):
        ops.compact_rows(torch.zeros((4, 4)), torch.zeros(4, dtype=torch.int64), i32(1), 2)

    density, ndc, z, dirs = torch.zeros((4, 4, 4)), torch.zeros((2, 3, 3)), torch.zeros((2, 3)), torch.zeros((2, 3))
    vol = torch.zeros((1, 8, 4, 4, 4), requires_grad=True)
    imgs, w2cs, Ks = torch.zeros((3, 3, 8, 8)), torch.eye(4).repeat(3, 1, 1), torch.eye(3).repeat(3, 1, 1)
    net = {k: models.MVSNeRF(D=6, W=w, input_ch_pts=63, input_ch_views=3, input_ch_feat=20, skips=[4], net_type=t)
           for k, w, t in (("v0", 128, "v0"), ("v2", 128, "v2"), ("wide", 256, "v0"))}
    call = lambda n, d=density, thr=0.0: ops.raymarch_sparse_train(vol, imgs, w2cs, Ks, n, ndc, ndc, z, dirs, d, thr)
    with pytest.raises(ValueError, match="NaN"):
        call(net["v0"], thr=float("nan"))
    with pytest.raises(RuntimeError, match=r"\(D,H,W\)"):
        call(net["v0"], d=torch.zeros((1, 1, 4, 4, 4)))
    with pytest.raises(NotImplementedError, match="netwidth 256"):
        call(net["wide"])
    with ops.mlp_precision("bf16x3"), pytest.raises(RuntimeError, match="'fp32' or 'bf16'"):
        call(net["v0"])
    with ops.mlp_precision("bf16"), pytest.raises(NotImplementedError, match="net_type v2"):
        call(net["v2"])
    # the render-only op next to it still has no backward
    with pytest.raises(NotImplementedError, match="no backward"):
        ops.raymarch_sparse(torch.zeros((4, 4, 4, 8), requires_grad=True), None, None, None, None, ndc, ndc, z, dirs, density, 0.0)

    # the systems, built without their constructors (those encode a scene)
    gen = train.MVSSystem.__new__(train.MVSSystem)
    torch.nn.Module.__init__(gen)
    gen.args = types.SimpleNamespace(skip_empty_train=0.0)
    with pytest.raises(ValueError, match="skip_empty_train"):
        gen.training_step({}, 0)
    ft = train.MVSSystemFinetune.__new__(train.MVSSystemFinetune)
    torch.nn.Module.__init__(ft)
    ft.imgs = torch.zeros((1, 3, 3, 8, 8))
    batch = {"rays": torch.zeros((1, 5, 8)), "rgbs": torch.zeros((1, 5, 3))}
    ft.args = types.SimpleNamespace(skip_empty_train=float("nan"))
    with pytest.raises(ValueError, match="NaN"):
        ft.training_step(batch, 0)
    ft.args = types.SimpleNamespace(skip_empty_train=0.0, skip_empty_refresh=0)
    with pytest.raises(ValueError, match="skip_empty_refresh"):
        ft.training_step(batch, 0)
    ft.args = types.SimpleNamespace(skip_empty_train=0.0)
    ft.global_step, ft.network_fn, ft.render_kwargs_train = 0, torch.nn.Linear(2, 2), {}              # not what create_nerf_mvs builds
    with pytest.raises(NotImplementedError, match="fused configuration"):
        ft.training_step(batch, 0)


def test_switch_defaults():
    from mvsnerf_amd import train
    assert not hasattr(train.default_args(), "skip_empty_train")                                 # read with getattr: default_args stays as it is
    assert train._skip_empty_train(types.SimpleNamespace()) is None
    assert train._skip_empty_train(types.SimpleNamespace(skip_empty_train=None)) is None
    assert train._skip_empty_train(types.SimpleNamespace(skip_empty_train=0)) == (0.0, 1, 200)
    assert train._skip_empty_train(types.SimpleNamespace(skip_empty_train=0.5, skip_empty_dilate=0, skip_empty_refresh=4)) == (0.5, 0, 4)
