"""The precision-recall entries' argument checks (include/gnnome_hip.h), which need no GPU: limits 1 <= E < 2^31, null pointers and the
workspace size are refused before anything is enqueued.  The compute side is tests/test_pr_curve_device.py (-m gpu)."""
import ctypes

from gnnome_amd import _lib, metrics


def test_sizes_and_limits():
    lib = _lib.load()
    T = metrics.pr_curve_tile_size()
    assert T >= 64 and T & (T - 1) == 0
    need, more = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.gnnome_pr_curve_workspace_bytes(1, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.gnnome_pr_curve_workspace_bytes((1 << 31) - 1, ctypes.byref(more)) == 0
    assert more.value >= 16 * (((1 << 31) - 1) // T)          # a 64-bit tile sum and a float64 partial per tile
    for bad in (0, -1, 1 << 31):
        assert lib.gnnome_pr_curve_workspace_bytes(bad, ctypes.byref(need)) == -1 and b"num_edges" in lib.gnnome_last_error()
    assert lib.gnnome_pr_curve_tile_size(None) == -1


def test_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    res = (ctypes.c_int64 * 4)()
    for bad in (0, 1 << 31):
        assert lib.gnnome_pr_curve_keys(one, one, bad, 0, 0, one, None, one, 1 << 20, None) == -1 and b"2^31" in lib.gnnome_last_error()
        assert lib.gnnome_pr_curve_scan(one, bad, one, 1 << 20, res, None) == -1 and b"2^31" in lib.gnnome_last_error()
        assert lib.gnnome_pr_curve_emit(one, bad, 1, 1, one, one, one, one, one, one, one, 1 << 20, None) == -1
        assert lib.gnnome_pr_curve_ap(one, one, bad, one, one, 1 << 20, None) == -1
    assert lib.gnnome_pr_curve_keys(one, one, 5000, 0, 0, one, None, one, 8, None) == -3 and b"workspace" in lib.gnnome_last_error()
    assert lib.gnnome_pr_curve_scan(one, 5000, one, 8, res, None) == -3
    assert lib.gnnome_pr_curve_emit(one, 5000, 10, 10, one, one, one, one, one, one, one, 8, None) == -3
    assert lib.gnnome_pr_curve_ap(one, one, 5000, one, one, 8, None) == -3
    assert lib.gnnome_pr_curve_keys(None, one, 5, 0, 0, one, None, one, 1 << 20, None) == -1 and b"null" in lib.gnnome_last_error()
    assert lib.gnnome_pr_curve_keys(one, one, 5, 0, 0, one, None, None, 1 << 20, None) == -1 and b"null" in lib.gnnome_last_error()
    assert lib.gnnome_pr_curve_scan(one, 5, one, 1 << 20, None, None) == -1 and b"null" in lib.gnnome_last_error()
    assert lib.gnnome_pr_curve_ap(one, None, 5, one, one, 1 << 20, None) == -1 and b"null" in lib.gnnome_last_error()
    for M, P in ((0, 1), (6, 1), (1, 0), (1, 6)):      # thresholds and positives outside [1, E]
        assert lib.gnnome_pr_curve_emit(one, 5, M, P, one, one, one, one, one, one, one, 1 << 20, None) == -1
        assert b"thresholds" in lib.gnnome_last_error()
