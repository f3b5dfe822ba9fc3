"""The launch coalescer's admit-or-flush decision (csrc/coalesce_admit.h)
through its binding: pure address arithmetic, no GPU."""
import ps_lite_amd as ps

_admit = ps._core.coalesce_admit
_KB = 1024
_BASE = 1 << 30  # any 16 B-aligned address; nothing is dereferenced


def _seg(i, nbytes=4 * _KB):
    """i-th of a family of pairwise disjoint segments (64 KiB apart)."""
    at = _BASE + i * 3 * 64 * _KB
    return (at, at + 64 * _KB, at + 128 * _KB, nbytes)


def test_disjoint_segments_are_admitted():
    assert _admit([], _seg(0)) == "admit"
    assert _admit([_seg(0), _seg(1), _seg(2)], _seg(3)) == "admit"
    # a shared SOURCE is no hazard: both only read it
    a = _seg(0)
    b = _seg(1)
    assert _admit([a], (b[0], b[1], a[2], a[3])) == "admit"
    # touching ranges do not overlap
    assert _admit([a], (a[0] + a[3], b[1], b[2], a[3])) == "admit"


def test_same_dst0_flushes():
    a, b = _seg(0), _seg(1)
    assert _admit([_seg(2), a], (a[0], b[1], b[2], b[3])) == "flush"
    # partial overlap, and the other destination
    assert _admit([a], (a[0] + 16, b[1], b[2], b[3])) == "flush"
    assert _admit([a], (b[0], a[1] + a[3] - 16, b[2], b[3])) == "flush"
    # a new destination over an earlier source
    assert _admit([a], (a[2], b[1], b[2], b[3])) == "flush"


def test_new_src_over_earlier_dst1_flushes():
    a, b = _seg(0), _seg(1)
    assert _admit([a], (b[0], b[1], a[1], b[3])) == "flush"
    assert _admit([a], (b[0], b[1], a[0] + 2 * _KB, b[3])) == "flush"


def test_misaligned_segment_is_rejected():
    a = _seg(0)
    for bad in ((a[0] + 4, a[1], a[2], a[3]), (a[0], a[1] + 8, a[2], a[3]),
                (a[0], a[1], a[2] + 1, a[3]), (a[0], a[1], a[2], a[3] + 12),
                (a[0], a[1], a[2], 0)):
        assert _admit([], bad) == "reject"
        assert _admit([_seg(1)], bad) == "reject"
    # its own ranges overlap
    assert _admit([], (a[0], a[0] + 16, a[2], a[3])) == "reject"


def test_65th_segment_is_rejected():
    full = [_seg(i) for i in range(64)]
    assert _admit(full[:63], _seg(63)) == "admit"
    assert _admit(full, _seg(64)) == "reject"
