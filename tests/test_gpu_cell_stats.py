"""GPU side of the per-cell statistics grid and the variance centre (ffl_cell_stats: k_cell_stats, k_grid_centre; DESIGN.md
section 17), everything through the C ABI via _capi, on fields placed with import_flows / upload_flow, and bit for bit
against the restatement tests/grid_ref.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import grid_ref as gr
from funscript_flow_amd import _capi

DEV = "cuda:0"
CELL, CEN = _capi.CELL_DTYPE.itemsize, _capi.GRID_CENTRE_DTYPE.itemsize
# (w, h, G): each the smallest shape that trips one mechanism of the kernel
SHAPES = [(16, 16, 16),     # one-pixel cells: every variance +0.0, empty = 1, the default centre
          (16, 16, 1),      # one cell covers the whole frame
          (53, 37, 5),      # odd width (rows not 16-byte aligned), remainder columns and rows
          (130, 33, 3),     # gh = 11, not a multiple of the rows in flight
          (300, 20, 3),     # the cell at columns 200..299 crosses the block edge at 256
          (600, 16, 1),     # one cell over three blocks
          (520, 16, 2),     # gw = 260: cells start and end inside different blocks
          (64, 64, 32),     # 2x2-pixel cells
          (256, 256, 32),   # the reference's operating point
          (192, 136, 64)]   # FFL_MAX_CELLS; gh = 2, gw = 3


def sid(s):
    return f"{s[0]}x{s[1]}-G{s[2]}"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def context(w, h, mb=8, slots=None):
    return _capi.Context(w, h, max_batch=mb, frame_slots=2, flow_slots=slots or 2 * mb)


@functools.lru_cache(maxsize=None)
def field(w, h, seed):
    f = gr.field(w, h, seed)
    f.setflags(write=False)
    return f


def want_bytes(f, G):
    """(cell records, centre record) of one field as the bytes ffl_cell_stats writes"""
    rec = np.ascontiguousarray(gr.cell_records(f, G))
    cx, cy, T, empty = gr.centre_of(rec[..., 3], f.shape[1], f.shape[0])
    cen = np.zeros(1, _capi.GRID_CENTRE_DTYPE)
    cen["cx"], cen["cy"], cen["total_var"], cen["cells"], cen["empty"] = cx, cy, T, G, empty
    return rec.tobytes(), cen.tobytes()


def run(ctx, slots, G, cells=True, centres=True, stream=None):
    """ffl_cell_stats into sentinel-filled buffers: (cell bytes or None, centre bytes or None)"""
    n = len(slots)
    co = torch.full((n * G * G * CELL,), 0xA5, dtype=torch.uint8, device=DEV) if cells else None
    ce = torch.full((n * CEN,), 0xA5, dtype=torch.uint8, device=DEV) if centres else None
    ctx.cell_stats(slots, G, co, ce, stream)
    return (co.cpu().numpy().tobytes() if cells else None), (ce.cpu().numpy().tobytes() if centres else None)


def rec_bytes(recs):
    return [(x, y, np.float32(d).tobytes(), np.float32(m).tobytes(), c) for x, y, d, m, c in recs]


# ---- 1. the shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_shapes_match_the_restatement(shape):
    w, h, G = shape
    assert _capi.cell_grid(w, h, G) == gr.geometry(w, h, G)
    fields = [field(w, h, 3 * w + i) for i in range(2)]
    with context(w, h, mb=4) as ctx:
        ctx.import_flows(dev(np.stack(fields)), [2, 1])
        cells, cen = run(ctx, [2, 1], G)
        want = [want_bytes(f, G) for f in fields]
        assert cells == b"".join(c for c, _ in want)
        assert cen == b"".join(c for _, c in want)
        rec = np.frombuffer(cen, _capi.GRID_CENTRE_DTYPE)
        assert (rec["cells"] == G).all()
        if G == 16:   # one-pixel cells: no variance anywhere
            assert (rec["empty"] == 1).all() and (rec["cx"] == w // 2).all() and (rec["cy"] == h // 2).all()
            assert rec["total_var"].tobytes() == np.zeros(2).tobytes()
        elif (w, h, G) != (16, 16, 1):
            assert (rec["empty"] == 0).all()
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 2. the margin and non-finite values ---------------------------------------------------------------------------------------
def test_margin_is_never_read_and_a_nan_stays_in_its_cell():
    w, h, G = 53, 37, 5
    f = field(w, h, 4)
    bad = f.copy()
    bad[35:, :] = np.nan         # rows 35, 36 and columns 50..52 belong to no cell
    bad[:, 50:] = 1e30
    with context(w, h) as ctx:
        ctx.upload_flow(0, f)
        ctx.upload_flow(1, bad)
        clean = run(ctx, [0], G)
        assert run(ctx, [1], G) == clean == want_bytes(f, G)
        inside = bad.copy()
        inside[7, 10, 0] = np.nan   # cell (1, 1)
        ctx.upload_flow(1, inside)
        cells, cen = run(ctx, [1], G)
        rec = np.frombuffer(cells, _capi.CELL_DTYPE).reshape(G, G)
        ref = np.frombuffer(clean[0], _capi.CELL_DTYPE).reshape(G, G)
        c = np.frombuffer(cen, _capi.GRID_CENTRE_DTYPE)[0]
        assert np.isnan(rec["var_mag"][1, 1]) and np.isnan(c["total_var"]) and np.isnan(c["cx"]) and np.isnan(c["cy"])
        assert c["empty"] == 0 and c["cells"] == G
        keep = np.ones((G, G), bool)
        keep[1, 1] = False
        assert rec[keep].tobytes() == ref[keep].tobytes()
        assert rec["mean_v"][1, 1].tobytes() == ref["mean_v"][1, 1].tobytes()   # v of that pixel is finite


# ---- 3. many items, either output, nothing else touched ---------------------------------------------------------------------
def test_five_items_either_output_and_nothing_else_changes():
    w, h, G = 130, 33, 3
    slots = [7, 2, 5, 0, 3]
    fields = [field(w, h, 40 + i) for i in range(5)]
    with context(w, h, mb=8) as ctx:
        ctx.import_flows(dev(np.stack(fields)), slots)
        flows = [ctx.download_flow(s).tobytes() for s in slots]
        recs = rec_bytes(ctx.pass1_results(slots, 1.0))
        both = run(ctx, slots, G)
        want = [want_bytes(f, G) for f in fields]
        assert both == (b"".join(c for c, _ in want), b"".join(c for _, c in want))
        assert run(ctx, slots, G, centres=False) == (both[0], None)
        assert run(ctx, slots, G, cells=False) == (None, both[1])
        assert run(ctx, slots[::-1], G) == (b"".join(c for c, _ in want[::-1]), b"".join(c for _, c in want[::-1]))
        assert [ctx.download_flow(s).tobytes() for s in slots] == flows
        assert rec_bytes(ctx.pass1_results(slots, 1.0)) == recs
        # another grid on the same slots through the same scratch
        assert run(ctx, slots[:2], 1) == tuple(b"".join(want_bytes(f, 1)[k] for f in fields[:2]) for k in (0, 1))
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 4. a large DC offset ------------------------------------------------------------------------------------------------------
def test_dc_offset_of_1e4_px():
    """the sums are taken about K, so an offset of 1e4 px costs the variance nothing; compared with the restatement alone (the
    reference's float32 variance is meaningless here)"""
    w, h, G = 80, 48, 8
    f = field(w, h, 9).copy()
    f[..., 0] += np.float32(1e4)
    f[..., 1] -= np.float32(6e3)
    with context(w, h) as ctx:
        ctx.upload_flow(3, f)
        got = run(ctx, [3], G)
        assert got == want_bytes(f, G)
        var = np.frombuffer(got[0], _capi.CELL_DTYPE)["var_mag"]
        assert (var >= 0).all() and var.max() < 10.0 and np.frombuffer(got[1], _capi.GRID_CENTRE_DTYPE)["empty"][0] == 0


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
class Span:
    """`nbytes` bytes at `ptr` as a __cuda_array_interface__ object, whatever memory that is"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"version": 2, "data": (int(ptr), False), "shape": (int(nbytes),), "strides": None,
                                         "typestr": "|u1"}


def test_refusals():
    w, h, G = 53, 37, 5
    INVALID, STATE = _capi.FFL_ERR_INVALID, _capi.FFL_ERR_STATE
    with _capi.Context(w, h, max_batch=4, frame_slots=2, flow_slots=8) as ctx:
        ctx.import_flows(dev(np.stack([field(w, h, 60 + i) for i in range(4)])), [0, 1, 2, 3])
        before = run(ctx, [0, 1, 2, 3], G)
        co = torch.full((5 * G * G * CELL,), 0xA5, dtype=torch.uint8, device=DEV)   # room for the five slots of a refused call
        ce = torch.full((5 * CEN,), 0xA5, dtype=torch.uint8, device=DEV)

        def refused(match, code, call):
            with pytest.raises(_capi.FFLError, match=match) as e:
                call()
            assert e.value.code == code and "ffl_cell_stats" in str(e.value)

        cs = lambda s, g=G, a=co, b=ce, stream=None: (lambda: ctx.cell_stats(s, g, a, b, stream))
        refused(r"n = 0 slots outside 1\.\.4", INVALID, cs([]))
        refused(r"n = 5 slots outside 1\.\.4", INVALID, cs([0, 1, 2, 3, 4]))
        refused(r"flow slot 8 out of range", INVALID, cs([8]))
        refused(r"flow slot 1 repeated in one call", INVALID, cs([0, 1, 1]))
        refused(r"flow slot 5 holds no flow", STATE, cs([0, 5]))
        refused(r"rule G1: cells = 0 outside 1\.\.64", INVALID, cs([0], 0, None, ce))
        refused(r"rule G1: cells = 65 outside 1\.\.64", INVALID, cs([0], 65, None, ce))
        refused(r"rule G1: cells = 38 exceeds min\(width, height\) of 53x37", INVALID, cs([0], 38, None, ce))
        refused(r"cells_dev and centres_dev are both NULL", INVALID, cs([0], G, None, None))
        refused(r"must be 8-byte aligned", INVALID, cs([0], G, Span(co.data_ptr() + 4, G * G * CELL), ce))
        refused(r"must be 8-byte aligned", INVALID, cs([0], G, co, Span(ce.data_ptr() + 4, CEN)))
        pin = ctx.pinned_frames(1, channels=1)
        assert pin.size >= CEN
        refused(r"centres_dev is page-locked host memory.*device memory", INVALID, cs([0], G, None, Span(pin.ctypes.data, CEN)))
        torch.cuda.empty_cache()
        big = torch.empty(18 << 20, dtype=torch.uint8, device=DEV)   # an allocation of its own
        past = Span(big.data_ptr() + big.numel() - 2 * G * G * CELL, 3 * G * G * CELL)
        refused(rf"cells_dev spans {3 * G * G * CELL} bytes, {G * G * CELL} more than its allocation holds", INVALID,
                cs([0, 1, 2], G, past, None))
        with pytest.raises(ValueError, match="cells_out holds"):
            ctx.cell_stats([0, 1], G, Span(co.data_ptr(), G * G * CELL), None)
        with pytest.raises(ValueError, match="not device memory"):
            ctx.cell_stats([0], G, None, torch.empty(CEN, dtype=torch.uint8))
        # a capturing stream; and a refused call queues nothing: the sentinels stand
        x = torch.zeros(16, device=DEV)
        g = torch.cuda.CUDAGraph()
        codes = []
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            try:
                cs([0], G, co, ce, torch.cuda.current_stream())()
            except _capi.FFLError as err:
                codes.append((err.code, "capturing" in str(err)))
            x += 1
        g.replay()
        torch.cuda.synchronize()
        assert codes == [(STATE, True)] and float(x.sum()) == 16.0
        assert (co.cpu().numpy() == 0xA5).all() and (ce.cpu().numpy() == 0xA5).all()
        assert run(ctx, [0, 1, 2, 3], G) == before
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 6. the stream contract ----------------------------------------------------------------------------------------------------
def test_stream_contract():
    """the outputs are read and then overwritten by work queued on the caller's stream right after the call, and the field
    that was imported is freed right after its import; no host synchronisation in between.  Once on torch's current stream,
    once on a second stream passed explicitly."""
    w, h, G = 130, 33, 3
    fields = [field(w, h, 70 + i) for i in range(3)]
    want = [want_bytes(f, G) for f in fields]
    with context(w, h) as ctx:
        for side in (None, torch.cuda.Stream()):
            torch.cuda.synchronize()
            with torch.cuda.stream(side if side is not None else torch.cuda.current_stream()):
                src = dev(np.stack(fields))
                co = torch.empty(3 * G * G * CELL, dtype=torch.uint8, device=DEV)
                ce = torch.empty(3 * CEN, dtype=torch.uint8, device=DEV)
                big = torch.ones(1 << 22, device=DEV)
                for _ in range(10):                               # keep the stream busy ahead of the calls
                    big = big * 1.0001
                co.fill_(0xA5)
                ce.fill_(0xA5)
                ctx.import_flows(src, [4, 5, 6], stream=side)
                del src                                           # freed right after the call
                junk = torch.full((3, h, w, 2), float("nan"), device=DEV)
                ctx.cell_stats([4, 5, 6], G, co, ce, side)
                a, b = co.clone(), ce.clone()
                co.zero_()                                        # overwritten behind the reader
                ce.zero_()
            (side or torch.cuda.current_stream()).synchronize()
            assert a.cpu().numpy().tobytes() == b"".join(c for c, _ in want)
            assert b.cpu().numpy().tobytes() == b"".join(c for _, c in want)
            assert not co.cpu().numpy().any() and not ce.cpu().numpy().any()
            del junk
        assert ctx.graph_stats()["capture_failures"] == 0
