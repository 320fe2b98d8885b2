"""The packed-weight cache of mvsnerf_amd/encoder.py (_PackedConv / _PackedConv2d) on the smallest layers that have each layout: when a getter
hands back the cached tensor and when it packs again, what the layouts hold, and how many re-layouts MVSNet.prepack batches into one launch."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda"

# job counts of the _PackBatch.launch calls of the second pass (weights epoch bumped after the first), recorded from the code before the getters
# were folded onto one lookup.  No-grad MVSNet.forward / training step (MVSNet.forward through _SweepRegFunction, then backward).
REPLAY_NO_GRAD = [19]
REPLAY_TRAIN = [37]


def _layers():
    torch.manual_seed(5)
    return {
        "c3s2": (nn.Conv3d(8, 16, 3, stride=2, padding=1, bias=False), False),
        "c3": (nn.Conv3d(16, 16, 3, padding=1, bias=False), False),
        "c44": (nn.Conv3d(44, 8, 3, padding=1, bias=False), False),
        "ct": (nn.ConvTranspose3d(16, 8, 3, padding=1, output_padding=1, stride=2, bias=False), True),
        "c2s2": (nn.Conv2d(8, 16, 5, stride=2, padding=2, bias=False), None),
        "c2": (nn.Conv2d(16, 16, 3, padding=1, bias=False), None),
    }


def _packed(name, weight=None):
    from mvsnerf_amd import encoder as E
    conv, transposed = _layers()[name]
    conv = conv.to(DEV)
    if weight is not None:
        with torch.no_grad():
            conv.weight.copy_(weight)
    return E._PackedConv2d(conv) if transposed is None else E._PackedConv(conv, transposed)


BOTH = [("fwd",), ("dgrad",)]
GETTERS = (
    [("c3s2", m, a) for m in ("get", "get_mfma", "get_bf16") for a in BOTH] + [("c3s2", "get_c8", ("fwd",)), ("c3s2", "get_f16x3", ())]
    + [("c3", m, a) for m in ("get", "get_mfma", "get_bf16") for a in BOTH] + [("c3", "get_f16x3", ())]
    + [("c44", "get", a) for a in BOTH] + [("c44", "get_c8", ("fwd",)), ("c44", "get_bf16", ("fwd",)), ("c44", "get_dgrad_slice", (12, 32)),
                                           ("c44", "get_bf16_conv0", ()), ("c44", "get_bf16_conv0", ((12, 32),)), ("c44", "get_f16x3_conv0", ())]
    + [("ct", m, a) for m in ("get", "get_c8", "get_mfma", "get_bf16") for a in BOTH]
    + [(n, m, a) for n in ("c2s2", "c2") for m in ("get", "get_bf16") for a in BOTH]
)


@pytest.mark.parametrize("name,method,args", GETTERS, ids=[f"{n}.{m}{a}" for n, m, a in GETTERS])
def test_hit_miss_and_contents(name, method, args):
    from mvsnerf_amd import _lib
    pk = _packed(name)
    call = lambda: getattr(pk, method)(*args)
    first = call()
    if first is None:                           # no kernel for this shape: nothing packed, nothing cached
        assert pk.cache == {}
        return
    assert len(pk.cache) == 1 and call() is first
    with torch.no_grad():
        pk.conv.weight.add_(1)
    second = call()
    assert second is not first and second.shape == first.shape and not torch.equal(second, first)
    assert call() is second
    _lib._bump_weights_epoch()                  # what an optimizer step does (a fused one leaves `_version` alone)
    third = call()
    assert third is not second and torch.equal(third, second) and call() is third
    pk.cache.clear()                            # MVSNet.invalidate_packed
    fourth = call()
    assert fourth is not third and torch.equal(fourth, third) and call() is fourth
    assert len(pk.cache) == 1
    fresh = getattr(_packed(name, pk.conv.weight), method)(*args)          # a cache that never missed twice, equal weights
    assert fresh is not fourth and torch.equal(fresh, fourth)


def test_fwd_layout_is_tap_cin_cout():
    pk = _packed("c3")
    assert torch.equal(pk.get("fwd").view(27, 16, 16), pk.conv.weight.detach().permute(2, 3, 4, 1, 0).reshape(27, 16, 16))


def test_dgrad_slice_has_one_slot(monkeypatch):
    from mvsnerf_amd import encoder as E
    packs = []
    real = E._pack
    monkeypatch.setattr(E, "_pack", lambda *a: packs.append(a[3:]) or real(*a))
    pk = _packed("c44")
    a = pk.get_dgrad_slice(0, 32)
    b = pk.get_dgrad_slice(4, 32)
    assert list(pk.cache) == ["dgrad_slice"] and pk.cache["dgrad_slice"][1] is b and pk.cache["dgrad_slice"][0][-2:] == (4, 32)
    assert pk.get_dgrad_slice(4, 32) is b and len(packs) == 2
    a2 = pk.get_dgrad_slice(0, 32)              # the first range again: packed again
    assert len(packs) == 3 and a2 is not a and torch.equal(a2, a) and not torch.equal(a, b)
    assert list(pk.cache) == ["dgrad_slice"] and pk.cache["dgrad_slice"][1] is a2
    # [27][cout][n] with mirrored taps of the layer's inputs 4 .. 35
    w = pk.conv.weight.detach()
    assert torch.equal(b.view(27, 8, 32), w[:, 4:36].flip(2, 3, 4).permute(2, 3, 4, 0, 1).reshape(27, 8, 32))
    with pytest.raises(RuntimeError):
        pk.get_dgrad_slice(16, 32)              # past the layer's 44 inputs
    with pytest.raises(RuntimeError):
        _packed("c3s2").get_dgrad_slice(0, 8)   # a strided layer
    assert len(packs) == 3


def test_conv2d_stride2_has_no_bf16_dgrad():
    pk = _packed("c2s2")                         # (its data gradient runs on the gather-form fp32 kernel)
    assert pk.get_bf16("fwd") is not None and list(pk.cache) == ["fwd_bf16"]
    assert pk.get_bf16("dgrad") is None and list(pk.cache) == ["fwd_bf16"]


def test_wrong_layer_raises_and_caches_nothing():
    pk = _packed("c3")
    for getter in (pk.get_bf16_conv0, pk.get_f16x3_conv0):
        with pytest.raises(RuntimeError):
            getter()
    assert pk.cache == {}


def _scene():
    from mvsnerf_amd import encoder as E
    from mvsnerf_amd.synth import make_rig
    torch.manual_seed(3)
    net = E.MVSNet().to(DEV).train()
    net.D = 8
    rig = make_rig(64, 96, seed=11, rot_deg=2.0)
    return net, rig["images"][:, :3].to(DEV), rig["proj_mats"][:, :3].to(DEV), rig["near_fars"][0, 0].to(DEV)


def _count_launches(monkeypatch):
    from mvsnerf_amd import encoder as E
    counts = []
    real = E._PackBatch.launch
    monkeypatch.setattr(E._PackBatch, "launch", staticmethod(lambda jobs: counts.append(len(jobs)) or real(jobs)))
    return counts


def test_replay_no_grad(monkeypatch):
    """The second encode packs every layout the first one asked for in ONE launch up front (MVSNet.prepack) and none on its own."""
    from mvsnerf_amd import _lib
    net, imgs, proj, nf = _scene()
    counts = _count_launches(monkeypatch)
    with torch.no_grad():
        net(imgs, proj, nf)
        first = list(counts)
        _lib._bump_weights_epoch()
        del counts[:]
        net(imgs, proj, nf)
    print("no-grad encode: first pass", first, "second pass", counts)
    assert counts == REPLAY_NO_GRAD


def test_replay_training_step(monkeypatch):
    from mvsnerf_amd import _lib
    net, imgs, proj, nf = _scene()
    counts = _count_launches(monkeypatch)
    net(imgs, proj, nf)[0].sum().backward()
    first = list(counts)
    _lib._bump_weights_epoch()
    del counts[:]
    vol = net(imgs, proj, nf)[0]
    assert type(vol.grad_fn).__name__.startswith("_SweepRegFunction")
    vol.sum().backward()
    print("training step: first pass", first, "second pass", counts)
    assert counts == REPLAY_TRAIN
