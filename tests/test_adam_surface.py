"""CPU-only: what mvsnerf_adam_step_multi refuses before any launch (csrc/adam.hip; the contract is the Adam paragraph of include/mvsnerf_hip.h).  Every call
here either is refused or has no element to update, so nothing is launched and host buffers are enough (as tests/test_scatter_det_surface.py does).  A job
that has to PASS its checks is shown to pass by what a later job of the same table is refused for: the checks run in table order."""
import ctypes

from mvsnerf_amd import _lib

OK, EINVAL, EUNSUPPORTED, EALIGN = 0, -1, -2, -3
SCAL = (5e-4, 0.9, 0.999, 1e-8, 0.03)


def _buf():
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert p % 16 == 0
    return buf, p


def _call(jobs, n=None):
    """jobs: [(p, g, m, v, numel)] with integer addresses."""
    k = len(jobs)
    arr = ctypes.c_void_p * max(k, 1)
    cols = [arr(*[j[c] for j in jobs]) for c in range(4)]
    numel = (ctypes.c_int64 * max(k, 1))(*[j[4] for j in jobs])
    return _lib.lib().mvsnerf_adam_step_multi(k if n is None else n, *cols, numel, *SCAL, 0)


def test_counts_and_tables():
    l = _lib.lib()
    buf, p = _buf()
    assert l.mvsnerf_adam_step_multi(0, None, None, None, None, None, *SCAL, 0) == OK           # nothing to do, no table needed
    assert l.mvsnerf_adam_step_multi(-1, None, None, None, None, None, *SCAL, 0) == EINVAL
    assert _call([(p, p, p, p, 0)], n=-1) == EINVAL
    arr, num = (ctypes.c_void_p * 1)(p), (ctypes.c_int64 * 1)(0)
    for null in range(5):                                                                       # each of the five tables
        a = [arr, arr, arr, arr, num]
        a[null] = None
        assert l.mvsnerf_adam_step_multi(1, *a, *SCAL, 0) == EINVAL, null
    assert l.mvsnerf_adam_step_multi(1, arr, arr, arr, arr, num, *SCAL, 0) == OK


def test_entries_of_the_tables():
    buf, p = _buf()
    for null in range(4):                                                                       # p, g, m, v of a job with elements
        j = [p, p, p, p, 5]
        j[null] = 0
        assert _call([tuple(j)]) == EINVAL, null
        assert _call([(p, p, p, p, 0), tuple(j)]) == EINVAL, null
    assert _call([(p, p, p, p, -1)]) == EINVAL and _call([(p, p, p, p, 0), (p, p, p, p, -4)]) == EINVAL
    assert _call([(p, p, p, p, 1 << 40)]) == EUNSUPPORTED and _call([(p, p, p, p, (1 << 40) + 3)]) == EUNSUPPORTED
    assert _call([(0, p, p, p, 1 << 40)]) == EINVAL                                             # an invalid argument is reported as such at that size
    # 2^30 workgroups of 1024 elements in one launch: two tensors of 2^39 elements are 2^30 together
    assert _call([(p, p, p, p, 1 << 39), (p, p, p, p, 1 << 39)]) == EUNSUPPORTED
    assert _call([(p, p, p, p, 1 << 39), (p, p, p, p, (1 << 39) - 1024), (p, p, p, p, 1)]) == EUNSUPPORTED
    # ... and a refusal comes before ANY launch, whichever trip of 84 jobs the refused job is in: 100 jobs of 5 elements at a null g
    assert _call([(p, p, p, p, 0)] * 90 + [(p, 0, p, p, 5)]) == EINVAL
    assert _call([(p, p, p, p, 0)] * 84 + [(p, p + 4, p, p, 8)]) == EALIGN
    assert _call([(p, p, p, p, 0)] * 200) == OK


def test_a_job_without_elements_is_not_looked_at():
    """The contract the header states: numel == 0 -> the four pointers are not read, so null and misaligned ones pass (a zero-element torch tensor has
    data_ptr() == 0); numel < 0 is still refused."""
    buf, p = _buf()
    assert _call([(0, 0, 0, 0, 0)]) == OK
    assert _call([(p, 0, p, p, 0), (p + 4, p + 8, p + 12, p + 4, 0), (0, 0, 0, 0, 0)]) == OK
    assert _call([(0, 0, 0, 0, 0), (0, 0, 0, 0, -1)]) == EINVAL
    assert _call([(0, 0, 0, 0, 0), (p, p, p, 0, 3)]) == EINVAL                                   # the job after it is still checked


def test_alignment_is_asked_of_whole_quad_tensors_only():
    buf, p = _buf()
    refused_later = (p, p, p, 0, 1)                  # a null v with an element: EINVAL, after every job before it has passed its checks
    for col in range(4):
        for off in (4, 8, 12):
            j = [p, p, p, p]
            j[col] = p + off
            for numel in (4, 8, 1024, 1 << 20):
                assert _call([(*j, numel)]) == EALIGN, (col, off, numel)
                assert _call([(p, p, p, p, 0), (*j, numel), refused_later]) == EALIGN
            for numel in (1, 2, 3, 5, 1023, 1025, (1 << 20) + 2):
                assert _call([(*j, numel), refused_later]) == EINVAL, (col, off, numel)          # passed: the answer is the next job's
    assert _call([(p + 16, p + 32, p + 48, p + 64, 4), refused_later]) == EINVAL                 # 16-byte aligned quads pass as well
    assert _call([(p + 2, p, p, p, 4)]) == EALIGN
