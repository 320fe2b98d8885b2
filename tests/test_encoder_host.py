"""Host glue of mvsnerf_amd/encoder.py that needs no GPU: the layout parameters of every layer's weight re-layouts, the per-thread
`num_batches_tracked` bookkeeping and the set of module-level switches."""
import threading

import pytest
import torch

from mvsnerf_amd import encoder as E

# (ci_real, co_real, ci_pad, co_pad, s_ci, s_co, flip) per layer as (mode "fwd", mode "dgrad"), recorded from the code before the getters
# were folded onto one lookup: _PackedConv._params for the 3-D layers, the tuple _PackedConv2d.get / _get_bf16_2d handed to _pack for the 2-D ones.
_COSTREG_BEHIND_CONV0 = [
    ((8, 16, 8, 16, 27, 216, 0), (16, 8, 16, 8, 216, 27, 0)),
    ((16, 16, 16, 16, 27, 432, 0), (16, 16, 16, 16, 432, 27, 1)),
    ((16, 32, 16, 32, 27, 432, 0), (32, 16, 32, 16, 432, 27, 0)),
    ((32, 32, 32, 32, 27, 864, 0), (32, 32, 32, 32, 864, 27, 1)),
    ((32, 64, 32, 64, 27, 864, 0), (64, 32, 64, 32, 864, 27, 0)),
    ((64, 64, 64, 64, 27, 1728, 0), (64, 64, 64, 64, 1728, 27, 1)),
    ((64, 32, 64, 32, 864, 27, 0), (32, 64, 32, 64, 27, 864, 0)),
    ((32, 16, 32, 16, 432, 27, 0), (16, 32, 16, 32, 27, 432, 0)),
    ((16, 8, 16, 8, 216, 27, 0), (8, 16, 8, 16, 27, 216, 0)),
]
PARAMS = {
    "costreg41": [((41, 8, 44, 8, 27, 1107, 0), (8, 41, 8, 44, 1107, 27, 1))] + _COSTREG_BEHIND_CONV0,
    "costreg47": [((47, 8, 48, 8, 27, 1269, 0), (8, 47, 8, 48, 1269, 27, 1))] + _COSTREG_BEHIND_CONV0,
    "featnet": [                       # the eight ConvBnReLU layers, then the 1x1 toplayer
        ((3, 8, 4, 8, 9, 27, 0), (8, 3, 8, 4, 27, 9, 1)),
        ((8, 8, 8, 8, 9, 72, 0), (8, 8, 8, 8, 72, 9, 1)),
        ((8, 16, 8, 16, 25, 200, 0), (16, 8, 16, 8, 200, 25, 0)),
        ((16, 16, 16, 16, 9, 144, 0), (16, 16, 16, 16, 144, 9, 1)),
        ((16, 16, 16, 16, 9, 144, 0), (16, 16, 16, 16, 144, 9, 1)),
        ((16, 32, 16, 32, 25, 400, 0), (32, 16, 32, 16, 400, 25, 0)),
        ((32, 32, 32, 32, 9, 288, 0), (32, 32, 32, 32, 288, 9, 1)),
        ((32, 32, 32, 32, 9, 288, 0), (32, 32, 32, 32, 288, 9, 1)),
        ((32, 32, 32, 32, 1, 32, 0), (32, 32, 32, 32, 32, 1, 1)),
    ],
}


def _packed_of(name):
    if name == "featnet":
        net = E.FeatureNet()
        return [lay._packed for lay in net._layers()] + [net._top_packed]
    return [lay._packed for lay in E.CostRegNet(int(name[-2:]))._layers()]


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_params_of_every_layer(name):
    packed = _packed_of(name)
    assert len(packed) == len(PARAMS[name])
    for i, (pk, (fwd, dgrad)) in enumerate(zip(packed, PARAMS[name])):
        assert pk._params("fwd") == fwd, (name, i)
        assert pk._params("dgrad") == dgrad, (name, i)
        # taps are mirrored for the data gradient of a stride-1 convolution only (a strided / transposed layer's gradient is the other kind of layer)
        stride1_conv = pk.conv.stride[0] == 1 and not getattr(pk, "transposed", False)
        assert pk._params("fwd")[6] == 0 and pk._params("dgrad")[6] == int(stride1_conv), (name, i)


def _counter():
    return torch.zeros((), dtype=torch.int64)


def test_nbt_counters_are_per_thread():
    """Thread A is inside _defer_nbt() (MVSNet.forward running FeatureNet) while thread B finishes a pass of its own: B's flush increments
    B's counter at once and leaves A's alone; A's flush after leaving the context increments A's only."""
    a, b = _counter(), _counter()
    a_inside, b_done = threading.Event(), threading.Event()
    seen, errors = {}, []

    def run(fn):
        try:
            fn()
        except BaseException as e:      # reported by the main thread
            errors.append(e)
            a_inside.set(); b_done.set()

    def thread_a():
        with E._defer_nbt():
            E._note_nbt(a)
            a_inside.set()
            assert b_done.wait(30)
            seen["a while deferring"] = int(a)
        E._flush_nbt()
        seen["a after A's flush"], seen["b after A's flush"] = int(a), int(b)

    def thread_b():
        assert a_inside.wait(30)
        E._note_nbt(b)
        E._flush_nbt()
        seen["b after B's flush"], seen["a after B's flush"] = int(b), int(a)
        b_done.set()

    threads = [threading.Thread(target=run, args=(f,)) for f in (thread_a, thread_b)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors, errors
    assert seen == {"b after B's flush": 1, "a after B's flush": 0, "a while deferring": 0, "a after A's flush": 1, "b after A's flush": 1}


def test_nbt_deferral_nests_on_one_thread():
    c = _counter()
    with E._defer_nbt():
        with E._defer_nbt():
            E._note_nbt(c)
            E._flush_nbt()
        E._flush_nbt()
        assert int(c) == 0              # still inside the outer deferral
    E._flush_nbt()
    assert int(c) == 1
    E._flush_nbt()
    assert int(c) == 1                  # flushed once, forgotten


def test_module_switches():
    for name in ("BF16_WGRAD", "BF16_LAYERS", "F16X3_LAYERS", "MATERIALIZE_UP_INPUT", "BLOCKED_COST"):
        assert not hasattr(E, name), name
    assert E.FUSED_ABN_STATS is True
    assert E.F16X3_MIN_VOXELS == 262144
    assert E.VOLUME_LAYOUT == "hwdc"
    assert E.PSW_BWD_DETERMINISTIC is False
    assert E.ENCODER_PRECISION == "auto"
    assert E._BLOCKED_CIN == (32, 36, 40, 44, 48, 52, 56)
