"""GPU sweep of the flow export (k_export_flows behind ffl_export_flows) at small shapes.  The ground
truth is the array that was uploaded, not a second device path: every slot is filled through upload_flow with a field whose
float32 bit patterns are all distinct per (slot, pixel, component) -- finite, with -0.0, denormals and +-FLT_MAX among them
-- download_flow is first checked to return those bits, and every export is then compared with them.  The context sizes are
chosen by what they do to the kernel's unit count (a block is 1024 units), the destinations by alignment and item stride;
every output buffer starts as a NaN-payload sentinel, and every word outside the written items must keep it.  Copy work:
bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from funscript_flow_amd import _capi

DEV = "cuda:0"
SENTINEL = 0x7FC5A5A5            # a quiet NaN with a payload: no field holds it, and arithmetic would not keep it
GUARD = 64                       # sentinel words before and after every destination (a multiple of 4: keeps 16-byte alignment)

# (w, h): N -- what the size exercises
SIZES = [(17, 19),   # 323: N odd -- scalar paths in both layouts even with an aligned dst
         (18, 17),   # 306: N % 4 == 2 -- NHWC vector, NCHW scalar
         (16, 16),   # 256: one partial block
         (64, 32),   # 2048: NHWC vector units = 1024, exactly one full block
         (41, 50),   # 2050: NHWC vector units = 1025, a second block with one unit
         (64, 64),   # 4096: NCHW vector units = 1024
         (65, 64)]   # 4160: NCHW vector units = 1040


def fields(n_slots, w, h, salt=0):
    """(n_slots, h, w, 2) uint32 bit patterns of finite float32 values, all distinct: the mantissa counts on from `salt`,
    the exponent (0..254, so denormals occur) and the sign vary with it.  salt == 0: -0.0, +-FLT_MAX, the smallest denormal
    and the smallest normal open slot 0, and the largest negative denormal and the neighbours of +-FLT_MAX close the last"""
    total = n_slots * h * w * 2
    assert total + salt < 1 << 22                         # the planted mantissas lie above every counted one
    i = np.arange(salt, salt + total, dtype=np.uint64)
    bits = ((i & np.uint64(1)) << np.uint64(31)) | ((i * np.uint64(37) % np.uint64(255)) << np.uint64(23)) | i
    bits = bits.astype(np.uint32)
    if salt == 0:
        bits[:5] = [0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x00800000]
        bits[-3:] = [0x807FFFFF, 0x7F7FFFFE, 0xFF7FFFFE]
        assert ((bits & 0x7F800000) == 0).sum() > 3       # denormals beside the three planted words with a zero exponent
    out = bits.reshape(n_slots, h, w, 2)
    assert np.isfinite(out.view(np.float32)).all() and len(np.unique(out)) == out.size
    return out


def fill(ctx, bits):
    """the fields into flow slots 0.., and the grounding: download_flow returns the uploaded bits"""
    for s, b in enumerate(bits):
        ctx.upload_flow(s, b.view(np.float32))
    for s, b in enumerate(bits):
        assert np.array_equal(ctx.download_flow(s).view(np.uint32), b), ("download_flow", s)


def item_bits(bits, slot, layout):
    b = bits[slot]
    return (b if layout == "nhwc" else b.transpose(2, 0, 1)).reshape(-1)


class Span:
    """n items of a sentinel-filled device buffer as a __cuda_array_interface__ object: item i starts `off + i * stride`
    words into the buffer (stride may be negative: the pointer is then to the last item in memory)"""

    def __init__(self, buf, off, stride, shape):
        inner = [4 * int(np.prod(shape[k + 1:])) for k in range(1, 4)]
        self.__cuda_array_interface__ = {"version": 2, "data": (buf.data_ptr() + 4 * off, False), "shape": tuple(shape),
                                         "strides": (4 * stride,) + tuple(inner), "typestr": "<f4"}


def export_into(ctx, bits, slots, layout, off, stride, words, what):
    """export `slots` to items `stride` words apart, the first `off` words into a buffer of `words` sentinel words; the
    whole buffer must then be the sentinel with the items' bits laid over it"""
    n, H, W = len(slots), ctx.height, ctx.width
    item = 2 * H * W
    buf = torch.full((words,), SENTINEL, dtype=torch.int32, device=DEV)
    want = np.full(words, SENTINEL, np.uint32)
    for i, s in enumerate(slots):
        lo = off + i * stride
        assert GUARD <= lo and lo + item <= words - GUARD
        want[lo:lo + item] = item_bits(bits, s, layout)
    shape = (n, H, W, 2) if layout == "nhwc" else (n, 2, H, W)
    ctx.export_flows(slots, Span(buf, off, stride, shape), layout=layout)
    got = buf.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, layout, f"{bad.size} words differ, the first at {bad[0]}: item offset "
                           f"{(bad[0] - off) % abs(stride) if stride else bad[0] - off}, got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_export_destinations_bit_exact_and_nothing_else_written(w, h, layout):
    N, item = w * h, 2 * w * h
    slots = [2, 0, 1]
    n = len(slots)
    with _capi.Context(w, h, max_batch=1, frame_slots=2, flow_slots=3) as ctx:
        bits = fields(3, w, h)
        fill(ctx, bits)
        # a fresh output
        fresh = ctx.export_flows(slots, layout=layout)
        assert tuple(fresh.shape) == ((n, h, w, 2) if layout == "nhwc" else (n, 2, h, w)) and fresh.dtype == torch.float32
        got = fresh.cpu().numpy().view(np.uint32).reshape(n, -1)
        for i, s in enumerate(slots):
            assert np.array_equal(got[i], item_bits(bits, s, layout)), ("fresh", i)
        assert torch.empty(1, device=DEV).data_ptr() % 16 == 0            # what "aligned" below rests on
        # back to back in a guarded buffer, 16-byte aligned when the item is
        export_into(ctx, bits, slots, layout, GUARD, item, 2 * GUARD + n * item, "contiguous")
        # every second item of a larger tensor
        export_into(ctx, bits, slots, layout, GUARD, 2 * item, 2 * GUARD + 2 * n * item, "every second item")
        # a dst that is only 4-byte aligned
        export_into(ctx, bits, slots, layout, GUARD + 1, item, 2 * GUARD + n * item + 4, "4-byte aligned dst")
        export_into(ctx, bits, slots, layout, GUARD + 2, item + 2, 2 * GUARD + n * (item + 2) + 4, "8-byte aligned dst")
        # a 16-byte aligned dst whose item stride is a multiple of 4 bytes but not of 16
        assert (item + 1) % 4
        export_into(ctx, bits, slots, layout, GUARD, item + 1, 2 * GUARD + n * (item + 1), "item stride % 16 != 0")
        if layout == "nchw":   # channel planes 1: of an (n, 3, H, W) tensor: plane 0 of every item keeps the sentinel
            export_into(ctx, bits, slots, layout, GUARD + N, 3 * N, 2 * GUARD + 3 * n * N, "planes 1: of (n, 3, H, W)")
        # a negative item stride: the pointer is to the last item in memory, and the items come out reversed
        gap = item + 4
        export_into(ctx, bits, slots, layout, GUARD + (n - 1) * gap, -gap, 2 * GUARD + n * gap, "negative item stride")
        export_into(ctx, bits, slots, layout, GUARD + (n - 1) * item, -item, 2 * GUARD + n * item, "negative, back to back")
        # one item: the stride is not used
        export_into(ctx, bits, [1], layout, GUARD, item, 2 * GUARD + item, "one item")


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_more_items_than_one_launch_holds(layout):
    """n = FFL_MAX_BATCH + 1 with repeated slots: the second chunk starts FFL_MAX_BATCH items on, whatever the stride's sign"""
    w = h = 16
    item, n = 2 * w * h, _capi.FFL_MAX_BATCH + 1
    slots = [i % 3 for i in range(n)]
    with _capi.Context(w, h, max_batch=1, frame_slots=2, flow_slots=3) as ctx:
        bits = fields(3, w, h)
        fill(ctx, bits)
        out = ctx.export_flows(slots, layout=layout)
        got = out.cpu().numpy().view(np.uint32).reshape(n, -1)
        for i in (255, 256, 0):
            assert np.array_equal(got[i], item_bits(bits, slots[i], layout)), i
        export_into(ctx, bits, slots, layout, GUARD, item, 2 * GUARD + n * item, "257 items")
        gap = item + 8
        export_into(ctx, bits, slots, layout, GUARD, gap, 2 * GUARD + n * gap, "257 items with gaps")
        export_into(ctx, bits, slots, layout, GUARD + (n - 1) * gap, -gap, 2 * GUARD + n * gap, "257 items, negative stride")


def test_repeated_slots_and_a_slot_just_rewritten():
    """a slot named several times in one call goes to every one of its items; an export queued right after upload_flow
    rewrote a slot sees the new field, and one queued before it saw the old (both on stream `post`)"""
    w, h = 18, 17
    item = 2 * w * h
    with _capi.Context(w, h, max_batch=1, frame_slots=2, flow_slots=2) as ctx:
        bits = fields(2, w, h)
        fill(ctx, bits)
        for layout in ("nhwc", "nchw"):
            export_into(ctx, bits, [1, 1, 0, 1], layout, GUARD, item, 2 * GUARD + 4 * item, "repeated slots")
        newer = fields(2, w, h, salt=1 << 20)
        assert not np.intersect1d(newer, bits).size
        before = ctx.export_flows([1, 0])                                   # no synchronisation from here ...
        ctx.upload_flow(1, newer[1].view(np.float32))
        after = ctx.export_flows([1, 0], layout="nchw")
        ctx.upload_flow(0, newer[0].view(np.float32))
        last = ctx.export_flows([0, 1, 0])                                  # ... to here
        b, a, l = (t.cpu().numpy().view(np.uint32) for t in (before, after, last))
        assert np.array_equal(b[0], bits[1]) and np.array_equal(b[1], bits[0])
        assert np.array_equal(a[0], newer[1].transpose(2, 0, 1)) and np.array_equal(a[1], bits[0].transpose(2, 0, 1))
        assert np.array_equal(l[0], newer[0]) and np.array_equal(l[1], newer[1]) and np.array_equal(l[2], newer[0])
        assert np.array_equal(ctx.download_flow(1).view(np.uint32), newer[1])
