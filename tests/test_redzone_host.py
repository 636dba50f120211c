"""The red-zone helpers of tests/helpers.py against a numpy byte arena standing in for the device: a clean run passes, and
one float written just before the payload, just after it, or into a pad channel is reported with its side and offset."""
import numpy as np
import pytest

import helpers


class _ArenaDevice:
    """malloc / h2d / d2h on a host byte arena; addresses start at a 256-aligned fake base like hipMalloc's."""
    BASE = 0x7F0000000000

    def __init__(self, size=8 << 20):
        self.mem = np.zeros(size, dtype=np.uint8)
        self.top = 0
        self.transfers = []

    def malloc(self, nbytes):
        p = self.top
        self.top += (max(int(nbytes), 16) + 255) // 256 * 256
        assert self.top <= self.mem.size
        return self.BASE + p

    def h2d(self, ptr, arr):
        raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        o = ptr - self.BASE
        assert 0 <= o and o + raw.size <= self.top
        self.mem[o:o + raw.size] = raw
        self.transfers.append(("h2d", raw.size))

    def d2h(self, ptr, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        o = ptr - self.BASE
        assert 0 <= o and o + n <= self.top
        return self.mem[o:o + n].copy().view(dtype).reshape(shape)

    def sync(self):
        pass

    def free(self, ptr):
        self.freed = getattr(self, "freed", []) + [ptr - self.BASE]

    def poke(self, ptr, value=1.5):
        self.h2d(ptr, np.array([value], np.float32))


class _HostTensor:
    """The fields of medicalseg_amd.device.Tensor that the helpers use."""

    def __init__(self, dev, ptr, n, d, h, w, c, ld, gen):
        self.dev, self.ptr, self.n, self.d, self.h, self.w, self.c, self.ld = dev, ptr, n, d, h, w, c, ld

    def numpy(self):
        full = self.dev.d2h(self.ptr, (self.n, self.d, self.h, self.w, self.ld), np.float32)
        return np.moveaxis(full[..., :self.c], -1, 1).copy()


@pytest.fixture
def arena(monkeypatch):
    a = _ArenaDevice()
    monkeypatch.setattr(helpers, "dev", lambda: a)
    monkeypatch.setattr(helpers, "_tensor", _HostTensor)      # no medicalseg_amd import: the HIP library need not be built
    monkeypatch.setattr(helpers, "_registry", [])
    monkeypatch.setattr(helpers, "_bases", {})
    return a


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_sentinel_is_a_quiet_nan_with_the_stated_bits():
    assert _bits(np.array([helpers.SENTINEL], np.float32))[0] == 0x7FC0BEEF
    assert np.isnan(helpers.SENTINEL)
    assert helpers.GUARD == 64 * 1024 and helpers.GUARD % 256 == 0


def test_clean_run_passes_and_empties_the_registry(arena):
    x = np.arange(2 * 3 * 2 * 2 * 3, dtype=np.float32).reshape(2, 3, 2, 2, 3)
    t = helpers.t_from_ncdhw(x, ld=5)
    e = helpers.t_empty(1, 3, 2, 2, 2, ld=4, fill=-3.0)
    v = helpers.vec(np.arange(7))
    p = helpers.dmalloc(40)
    assert len(helpers._registry) == 4
    for ptr in (t.ptr, e.ptr, v, p):
        assert ptr % 256 == 0
    # what a kernel may legitimately do: write the channels, the vector, the raw buffer
    arena.h2d(v, np.ones(7, np.float32))
    arena.h2d(p, np.zeros(10, np.float32))
    arena.h2d(e.ptr, np.array([1, 2, 3], np.float32))
    helpers.assert_redzones_intact()
    assert helpers._registry == []
    helpers.assert_redzones_intact()          # nothing registered: a no-op
    # payloads arrived as given; pad channels of an uploaded tensor are SENTINEL, those of a filled one hold the fill
    full = arena.d2h(t.ptr, (2, 2, 2, 3, 5), np.float32)
    assert np.array_equal(full[..., :3], np.moveaxis(x, 1, -1))
    assert np.all(_bits(full[..., 3:]) == helpers.SENTINEL_BITS)
    assert np.array_equal(arena.d2h(e.ptr, (8, 4), np.float32)[1:], np.full((7, 4), -3.0, np.float32))
    assert np.array_equal(helpers.vec_back(v, 7), np.ones(7, np.float32))


def test_one_allocation_and_one_fill_per_buffer(arena):
    helpers.dmalloc(1000)
    assert arena.top == helpers.GUARD + 1024 + helpers.GUARD
    assert arena.transfers == [("h2d", arena.top)]
    helpers.assert_redzones_intact()


def test_unfilled_t_empty_reads_back_all_sentinel(arena):
    t = helpers.t_empty(2, 3, 2, 3, 4, ld=5)
    got = arena.d2h(t.ptr, (2 * 2 * 3 * 4 * 5,), np.uint32)
    assert np.all(got == helpers.SENTINEL_BITS)
    assert np.isnan(helpers.t_to_ncdhw(helpers.t_empty(1, 2, 1, 2, 2))).all()
    helpers.assert_redzones_intact()


def _report(arena):
    with pytest.raises(AssertionError) as ei:
        helpers.assert_redzones_intact()
    assert helpers._registry == []            # cleared even when the check fails
    return str(ei.value)


def test_write_just_before_the_payload_is_a_head_corruption(arena):
    p = helpers.dmalloc(40)
    arena.poke(p - 4)
    msg = _report(arena)
    assert "head red zone" in msg and "tail red zone" not in msg and "pad red zone" not in msg
    assert "1 word(s)" in msg and "first at payload-4," in msg and "last at payload-4" in msg
    assert "test_redzone_host.py" in msg and "dmalloc(40)" in msg


def test_write_at_payload_plus_nbytes_is_a_tail_corruption(arena):
    # 40 bytes round up to 256: the element right after the payload lies inside the rounded size and must still be caught
    v = helpers.vec(np.zeros(10))
    arena.poke(v + 40)
    arena.poke(v + 40 + 300)
    msg = _report(arena)
    assert "tail red zone" in msg and "head red zone" not in msg
    assert "2 word(s)" in msg and "first at payload+40," in msg and "last at payload+340" in msg
    assert "vec(10)" in msg


def test_write_into_a_pad_channel_is_a_pad_corruption(arena):
    t = helpers.t_empty(1, 3, 2, 2, 2, ld=5, fill=-3.0)
    arena.poke(t.ptr + 4 * (6 * 5 + 4))       # voxel 6, channel 4
    arena.poke(t.ptr + 4 * (2 * 5 + 3))       # voxel 2, channel 3
    arena.poke(t.ptr + 4 * (2 * 5 + 1))       # voxel 2, channel 1: a real channel, not reported
    msg = _report(arena)
    assert "pad red zone" in msg and "head red zone" not in msg and "tail red zone" not in msg
    assert "2 word(s)" in msg and "first at payload+%d," % (4 * 13) in msg and "last at payload+%d" % (4 * 34) in msg
    assert "c=3" in msg and "ld=5" in msg and "(1, 2, 2, 2)" in msg


def test_rewriting_a_pad_with_the_same_value_but_other_bits_is_seen(arena):
    t = helpers.t_empty(1, 1, 1, 1, 2, ld=2, fill=0.0)
    arena.poke(t.ptr + 4, -0.0)               # compares equal as float, differs as uint32
    assert "pad red zone" in _report(arena)


def test_pads_owned_false_skips_the_pads_but_not_the_guards(arena):
    t = helpers.t_empty(1, 3, 1, 1, 2, ld=4, fill=0.0, pads_owned=False)
    arena.poke(t.ptr + 4 * 3)
    helpers.assert_redzones_intact()
    t = helpers.t_empty(1, 3, 1, 1, 2, ld=4, fill=0.0, pads_owned=False)
    arena.poke(t.ptr + 4 * 8)
    assert "tail red zone" in _report(arena)


def test_every_corrupted_buffer_is_listed(arena):
    a, b = helpers.dmalloc(16), helpers.dmalloc(16)
    arena.poke(a - 8)
    arena.poke(b + 16)
    msg = _report(arena)
    assert len(msg.splitlines()) == 2 and "head red zone" in msg and "tail red zone" in msg


def test_dfree_checks_frees_the_whole_allocation_and_rejects_foreign_pointers(arena):
    p = helpers.dmalloc(64)
    helpers.dfree(p)
    assert arena.freed == [0] and helpers._registry == []
    with pytest.raises(AssertionError, match="not the payload of a live guarded allocation"):
        helpers.dfree(p)                       # freed before
    with pytest.raises(AssertionError, match="not the payload of a live guarded allocation"):
        helpers.dfree(arena.malloc(64))        # never guarded
    q = helpers.dmalloc(64)
    arena.poke(q + 64)
    with pytest.raises(AssertionError, match="tail red zone"):
        helpers.dfree(q)
    assert len(arena.freed) == 2               # freed all the same
