#!/usr/bin/env python3
"""Drain timeline of the three level-0 k_blur_solve launches from a -DFFL_STAMP build (diagnostic only, never the shipped
code path): every workgroup leaves the device-wide clock at entry and exit; from these, the resident workgroups over time
and the slot-time a launch leaves empty -- in all, and in its drain, the span after its last workgroup has started -- as a
share of slots x launch time.  One configuration per process (the stamps of the last step stay in the device array).
Usage: FFL_LIB=/path/to/stamp/libffl_hip.so python profiles/tools/k5_drain.py [taper=1] [pairs=P] [minwgs=N] [rows=N]
       env WHB=1920,1080,32 (level 0 must be at least 1024 wide); built + run by profiles/tools/k5_stamps.sh"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from funscript_flow_amd import _capi  # noqa: E402
from funscript_flow_amd.synth import sine_translate_frames  # noqa: E402

if os.environ.get("FFL_LIB"):
    _capi.LIB_PATH = os.path.abspath(os.environ["FFL_LIB"])
W, H, B = (int(v) for v in os.environ.get("WHB", "1920,1080,32").split(","))
DRAIN_MAX, TICK_US = 8192, 0.01          # FFL_DRAIN_MAX; wall_clock64 counts at 100 MHz
NAMES = {"taper": "blur_taper", "pairs": "blur_taper_pairs", "minwgs": "blur_min_wgs", "rows": "blur_rows"}
cfg = dict(kv.split("=") for kv in sys.argv[1:])
fr = sine_translate_frames(B + 1, W, H, seed=1)
_capi.set_option("lanes", 1)
_capi.set_option("graph", 0)
with _capi.Context(W, H, frame_slots=B + 2, flow_slots=B, max_batch=B) as ctx:
    for k, v in cfg.items():
        ctx.set_option(NAMES[k], int(v))
    ctx.upload_frames(0, list(fr))
    for _ in range(3):
        ctx.flow_pairs(list(range(B)), list(range(1, B + 1)), list(range(B)))
    ctx.sync()
    out = (C.c_ulonglong * (3 * DRAIN_MAX * 2))()
    L = _capi.load()
    L.ffl_debug_read_drain.argtypes = [C.c_void_p]
    assert L.ffl_debug_read_drain(out) == 0
    occ = (C.c_int * 4)()           # resident workgroups per instantiation, from the library's own occupancy query
    L.ffl_debug_blur_slots.argtypes = [C.c_void_p]
    assert L.ffl_debug_blur_slots(occ) == 0
    opts = {k: ctx.get_option(k) for k in ("blur_rows", "blur_min_wgs", "blur_taper", "blur_taper_pairs", "tile_order")}
a = np.array(out, np.int64).reshape(3, DRAIN_MAX, 2)
print(f"{W}x{H} B={B} {cfg or 'defaults'}: slots {occ[0]} / {occ[2]} / {occ[3]}")
for kind, (name, slots) in enumerate((("folded first", occ[0]), ("fused update", occ[2]), ("last", occ[3]))):
    t = a[kind][(a[kind] != 0).all(axis=1)]
    if not len(t):
        print(f"  {name}: no stamps")
        continue
    grid = _capi.blur_plan((W + 63) // 64, (H + 15) // 16, B, slots, blocks=False, **opts)[1]
    if grid > DRAIN_MAX:
        print(f"  NOTE {name}: {grid} workgroups, only the first {DRAIN_MAX} (FFL_DRAIN_MAX) are stamped -- the shares below "
              "come from that subset and are not the launch's")
    t0, t1 = t[:, 0].min(), t[:, 1].max()
    t = (t - t0) * TICK_US
    T, life = (t1 - t0) * TICK_US, t[:, 1] - t[:, 0]
    last_start = t[:, 0].max()
    in_drain = np.clip(t[:, 1], last_start, None) - np.clip(t[:, 0], last_start, None)
    drain_empty = slots * (T - last_start) - in_drain.sum()
    ev = np.concatenate([np.stack([t[:, 0], np.ones(len(t))], 1), np.stack([t[:, 1], -np.ones(len(t))], 1)])
    ev = ev[np.argsort(ev[:, 0], kind="stable")]
    resident = np.cumsum(ev[:, 1])
    full = ev[np.argmax(resident >= 0.95 * resident.max()), 0]
    print(f"  {name:12s} {len(t)} workgroups on {slots} slots (peak resident {int(resident.max())}): launch {T:.0f} us, "
          f"workgroup life {np.median(life):.0f} us median ({life.min():.0f}..{life.max():.0f}); 95 % of the peak resident after "
          f"{full:.0f} us; last start at {last_start:.0f} us, drain {T - last_start:.0f} us; empty slot-time "
          f"{100 * (1 - life.sum() / (slots * T)):.1f} % of slots x launch, in the drain {100 * drain_empty / (slots * T):.1f} %")
    edges = np.linspace(0, T, 21)
    occ = [((np.clip(t[:, 1], lo, hi) - np.clip(t[:, 0], lo, hi)).sum() / (slots * (hi - lo))) for lo, hi in zip(edges, edges[1:])]
    print("    resident / slots per 5 % of the launch: " + " ".join(f"{100 * o:.0f}" for o in occ))
