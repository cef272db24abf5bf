"""GPU parity at the sizes and options BASELINE.json names and bench.py times -- through the C ABI.

  configs[1]  1920x1080, B = 32, library-default options (the folded first iteration on levels 0-1, strip walk of
              8 tiles, merged frame expansion): the exact path the driver's bench line comes from
  configs[2]  3840x2160, B = 32
  configs[3]  8 x 1080p clips over 8 ranks (here: 8 shard engines on the one GPU of the test box)
  configs[4]  5760x2880 side-by-side stereo, each 2880x2880 eye an independent image (FF:1074-1083)

Oracle runs are bounded to a few pairs per size (1 s at 1080p, 4 s at 4K / 2880^2 per pair and core); everything
else is checked against goldens made by the oracle in the build container (tests/golden/bench_*.json) and through
size-independent properties (reductions = the numpy restatement applied to the device's own flow; identical inputs
at different batch positions give identical bits)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as orc
import post_ref as pr
import golden_check
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench_batch(ctx, frames, B):
    """one bench.py step: B pairs of a B+1-frame stream, pass 1, centre smoothing inside the batch, pass 2"""
    for i in range(B + 1):
        ctx.upload_frame(i, frames[i])
    slots = list(range(B))
    ctx.flow_pairs(list(range(B)), list(range(1, B + 1)), slots)
    recs = ctx.pass1_results(slots, 7.0)
    centers = pipeline.smooth_centers([(r[0], r[1]) for r in recs])
    dots = ctx.radial(slots, centers, [r[4] for r in recs], False)
    return recs, dots


def _require_golden_match(status, detail):
    """check_batch returns None when this machine's numpy / libm rounds the synthetic texture differently from the
    build container's (the golden then describes other inputs): that is a SKIP of the golden half, never a silent pass."""
    if status is None:
        pytest.skip(f"golden comparison not possible here: {detail}")
    assert status is True, detail


def _check_reductions_on_own_flow(ctx, j, rec, flow):
    ox, oy, ov = orc.max_divergence_np(flow)
    assert (rec[0], rec[1]) == (ox, oy) and np.float32(rec[2]).tobytes() == np.float32(ov).tobytes(), j
    rm = float(orc.mean_mag_np(flow))
    assert abs(float(rec[3]) - rm) <= 1e-4 * rm, j
    pr.check_mean_mag(rec[3], flow)


@pytest.mark.parametrize("lanes", [1, 2])
def test_shipped_configuration_1080p_b32_against_oracle(lanes):
    """bench.py's step (B = 32, default fuse_first / blur_rows / merge_expand; lanes = 1 is the bench's setting,
    2 the library default): all 32 records and scalars against the oracle goldens, three flow fields bit for bit
    against the oracle run here, the other 29 through their crc or the period-16 property."""
    W, H, B = 1920, 1080, 32
    frames = sine_translate_frames(B + 1, W, H, seed=1)
    gold = golden_check.load_golden(W, H, B, 1)
    assert gold is not None
    try:
        _capi.set_option("lanes", lanes)
        with _capi.Context(W, H, frame_slots=B + 2, flow_slots=3 * B, max_batch=B) as ctx:
            recs, dots = _run_bench_batch(ctx, frames, B)
            flows = {j: ctx.download_flow(j) for j in range(B)}
            recs2, dots2 = _run_bench_batch(ctx, frames, B)            # the same step again: replayed from the graph
            gs = ctx.graph_stats()
    finally:
        _capi.set_option("lanes", 2)
    # the standard step runs from a captured hipGraph; a capture that fails would make it silently slower, never wrong
    assert gs["capture_failures"] == 0 and gs["captured"] >= 1 and gs["replayed"] == 2, gs
    assert [tuple(r) for r in recs2] == [tuple(r) for r in recs] and dots2 == dots
    status, detail = golden_check.check_batch(gold, frames, recs, dots, lambda j: flows[j])
    _require_golden_match(status, detail)
    for j in (0, B // 2 - 1, B - 1):                                   # first, middle, last pair of the batch
        assert np.array_equal(flows[j], orc.farneback(frames[j], frames[j + 1])), j
    for j in range(B):
        _check_reductions_on_own_flow(None, j, recs[j], flows[j])
    for j in range(B - 16):                                            # frames repeat with period 16
        assert np.array_equal(flows[j], flows[j + 16]) and tuple(recs[j]) == tuple(recs[j + 16]), j


def test_4k_b32_against_oracle():
    W, H, B = 3840, 2160, 32
    frames = sine_translate_frames(B + 1, W, H, seed=1)
    gold = golden_check.load_golden(W, H, B, 1)
    assert gold is not None
    try:
        _capi.set_option("lanes", 1)
        with _capi.Context(W, H, frame_slots=B + 2, flow_slots=B, max_batch=B) as ctx:
            recs, dots = _run_bench_batch(ctx, frames, B)
            status, detail = golden_check.check_batch(gold, frames, recs, dots, ctx.download_flow)
            _require_golden_match(status, detail)
            f5 = ctx.download_flow(5)
            assert np.array_equal(f5, orc.farneback(frames[5], frames[6]))      # one pair against the oracle here
            for j in range(0, B - 16, 3):
                a, b = ctx.download_flow(j), ctx.download_flow(j + 16)
                assert np.array_equal(a, b), j
                _check_reductions_on_own_flow(ctx, j, recs[j], a)
                assert tuple(recs[j]) == tuple(recs[j + 16])
    finally:
        _capi.set_option("lanes", 2)


def test_every_rank_clip_of_the_scaling_bench_against_goldens():
    """bench.py --gpus N gives rank r the clip of seed 10 + r (weak scaling, configs[3]).  The driver's 8-GPU node is the
    only place ranks 2..7 ever run, so their goldens (tests/golden/bench_1920x1080_b32_s10..17.json) are compared here on
    the one GPU of the test box: the exact bench step per clip, 32 records + 32 scalars + 3 flow crc32 each."""
    from concurrent.futures import ThreadPoolExecutor
    W, H, B = 1920, 1080, 32
    seeds = list(range(10, 18))
    with ThreadPoolExecutor(8) as ex:
        clips = list(ex.map(lambda sd: sine_translate_frames(B + 1, W, H, seed=sd), seeds))
    compared = 0
    try:
        _capi.set_option("lanes", 1)
        with _capi.Context(W, H, frame_slots=B + 2, flow_slots=B, max_batch=B) as ctx:
            for sd, frames in zip(seeds, clips):
                gold = golden_check.load_golden(W, H, B, sd)
                assert gold is not None, sd
                recs, dots = _run_bench_batch(ctx, frames, B)
                status, detail = golden_check.check_batch(gold, frames, recs, dots, ctx.download_flow)
                assert status is not False, (sd, detail)
                compared += status is True
    finally:
        _capi.set_option("lanes", 2)
    if compared == 0:
        pytest.skip("no clip's synthetic frames match the goldens on this machine (numpy/libm rounding)")
    assert compared == len(seeds)


def test_config4_stereo_5760x2880_split_per_eye():
    """configs[4]: the two 2880x2880 eyes of a 5760x2880 side-by-side frame go to the device straight out of the
    full frame (row stride 5760, no host copy); left eye bit-exact against the oracle, right eye through the
    reductions on its own flow; both eyes of both frames in ONE batch of independent pairs."""
    EW, EH = 2880, 2880
    full = sine_translate_frames(2, 2 * EW, EH, seed=2)                   # (2, 2880, 5760)
    with _capi.Context(EW, EH, max_batch=2, frame_slots=4, flow_slots=2) as ctx:
        for eye in (0, 1):
            for t in (0, 1):
                view = full[t][:, eye * EW:(eye + 1) * EW]
                assert not view.flags["C_CONTIGUOUS"] and view.strides[0] == 2 * EW
                ctx.upload_frame(2 * eye + t, view)
        ctx.flow_pairs([0, 2], [1, 3], [0, 1])
        recs = ctx.pass1_results([0, 1], 7.0)
        left, right = ctx.download_flow(0), ctx.download_flow(1)
        ref = orc.farneback(np.ascontiguousarray(full[0][:, :EW]), np.ascontiguousarray(full[1][:, :EW]))
        assert np.array_equal(left, ref)
        for j, f in ((0, left), (1, right)):
            _check_reductions_on_own_flow(ctx, j, recs[j], f)
            c = (0.45 * EW, 0.52 * EH)
            got = ctx.radial([j], [c], [False], False)[0]
            want = float(orc.radial_np(f, c, False, False))
            assert abs(got - want) <= 1e-4 * max(abs(want), 1e-6 * EW)
            pr.check_radial(got, f, c, False)
        assert not np.array_equal(left, right)
        # the same eye through a contiguous copy gives the same bits (the stride path changes nothing)
        ctx.upload_frame(0, np.ascontiguousarray(full[0][:, EW:]))
        ctx.upload_frame(1, np.ascontiguousarray(full[1][:, EW:]))
        ctx.flow_pairs([0], [1], [0])
        assert np.array_equal(ctx.download_flow(0), right)


def test_config3_eight_1080p_clips_over_eight_shard_engines():
    """configs[3] on one GPU: 8 clips (seeds 10..17, as bench.py --gpus 8 gives its ranks) x 1080p.
    (a) weak form (one clip per rank, what bench.py times): rank r's HipShardEngine on its own context gives the
        scalars of a plain PairEngine run of clip r;
    (b) one clip's pairs dealt over the 8 engines round-robin (BASELINE's wording) and in contiguous blocks: the
        gathered scalars equal the single-engine run; one pair against the oracle."""
    W, H, n_pairs, R, B = 1920, 1080, 8, 8, 4
    clips = [sine_translate_frames(n_pairs + 1, W, H, seed=10 + r, zoom=0.02) for r in range(R)]
    ctxs = [_capi.Context(W, H, max_batch=B, frame_slots=2 * B + 2, flow_slots=pipeline.min_flow_slots(B)) for _ in range(R)]
    try:
        single = []
        for r in range(R):
            dots, recs = pipeline.PairEngine(ctxs[r]).process_chunk(clips[r])
            single.append((dots, np.array([[x[0], x[1], int(x[4])] for x in recs], np.int64)))
        engines = [pipeline.HipShardEngine(c) for c in ctxs]
        for r in range(R):                                                # (a) a clip per rank
            dots, allrecs = pipeline.process_chunk_sharded(engines[r], clips[r], 0, 1, lambda o: [o])
            assert np.array_equal(dots, single[r][0]) and np.array_equal(allrecs, single[r][1]), r
        for assign, block in (("round_robin", 1), ("round_robin", 2), ("contiguous", 1)):   # (b) a clip over 8 ranks
            dots, allrecs = pipeline.process_chunk_local_ranks(engines, clips[3], assign=assign, block=block)
            assert np.array_equal(dots, single[3][0]) and np.array_equal(allrecs, single[3][1]), (assign, block)
        # after the contiguous run rank 5 holds pair 5 of clip 3 in its flow slot 0
        assert np.array_equal(ctxs[5].download_flow(0), orc.farneback(clips[3][5], clips[3][6]))
    finally:
        for c in ctxs:
            c.close()


_RANK_WORKER = r"""
import os, sys
import numpy as np
import torch.distributed as dist
sys.path.insert(0, {root!r})
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
frames = sine_translate_frames(22, 320, 180, seed=4, amp=(3.0, 2.0), period=9, zoom=0.02)
def allgather(obj):
    out = [None] * world
    dist.all_gather_object(out, obj)
    return out
res = []
with _capi.Context(320, 180, device=0, max_batch=4, frame_slots=10, flow_slots=21) as ctx:   # both ranks on cuda:0
    eng = pipeline.HipShardEngine(ctx)
    for assign, block in (("contiguous", 1), ("round_robin", 1), ("round_robin", 4)):
        dots, recs = pipeline.process_chunk_sharded(eng, frames, rank, world, allgather, assign=assign, block=block)
        res.append(np.concatenate([dots, recs.reshape(-1).astype(np.float64)]))
    # streaming form: pass 2 of interior pairs beside pass 1, only the 6 + 6 halo records cross between the passes
    dots, recs = pipeline.process_chunk_sharded_halo(eng, frames, rank, world, allgather)
    res.append(np.concatenate([dots, recs.reshape(-1).astype(np.float64)]))
if rank == 0:
    np.save({out!r}, np.stack(res))
dist.barrier()
dist.destroy_process_group()
"""


def test_two_ranks_on_one_device_under_gloo(tmp_path):
    """The N > 1 path with real devices: two processes (torch.distributed.run, gloo), each with its own context
    on cuda:0, run process_chunk_sharded under every assignment; the gathered result equals the single-rank run."""
    out = str(tmp_path / "res.npy")
    script = tmp_path / "rank_worker.py"
    script.write_text(_RANK_WORKER.format(root=ROOT, out=out))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                           "--master-addr", "127.0.0.1", "--master-port", "29573", str(script)], env=env, timeout=600)
    got = np.load(out)
    frames = sine_translate_frames(22, 320, 180, seed=4, amp=(3.0, 2.0), period=9, zoom=0.02)
    with _capi.Context(320, 180, max_batch=4, frame_slots=10, flow_slots=21) as ctx:
        dots, recs = pipeline.PairEngine(ctx).process_chunk(frames)
    want = np.concatenate([dots, np.array([[r[0], r[1], int(r[4])] for r in recs], np.float64).reshape(-1)])
    for g in got:
        assert np.array_equal(g, want)
    j = 13
    with _capi.Context(320, 180, max_batch=1) as ctx:
        ctx.submit_pair(0, frames[j], frames[j + 1])
        assert np.array_equal(ctx.download_flow(0), orc.farneback(frames[j], frames[j + 1]))


def test_bench_launches_its_own_ranks_from_a_plain_shell():
    """The driver's command form: `python bench.py --gpus 2 ...` with NO torch.distributed environment.  bench.py must
    become the parent that spawns the two rank processes (FF:1190-1191), and print exactly one JSON line with n_gpus 2,
    checked against the rank clips' goldens.  On this 1-GPU box the ranks share cuda:0 (--rehearse-gloo); without that
    flag two ranks on one card must end with status 3, one FATAL message and no JSON line."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full"]
    r = subprocess.run(cmd + ["--rehearse-gloo"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["scaling"] == "weak" and line["value"] > 0
    assert line["checked"] is True, line["check_detail"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 3 and r.stdout.strip() == "", (r.returncode, r.stdout)
    assert r.stderr.count("FATAL") == 1 and "drive the same GPU" in r.stderr, r.stderr[-2000:]


def test_batches_above_eight_pairs_small_sizes():
    """Batches of 17 .. 64 pairs at sizes where the oracle covers every pair (no parity test used a batch
    above 8), with the library's default fold threshold and with thresholds that fold every / some levels."""
    for (w, h, B, fuse) in [(640, 360, 32, 10000), (640, 360, 32, 1), (256, 256, 64, 10000), (200, 120, 17, 2000),
                            (256, 256, 256, 10000), (96, 80, 200, 10000)]:
        frames = sine_translate_frames(B + 1, w, h, seed=1, zoom=0.01)
        try:
            _capi.set_option("fuse_first", fuse)
            with _capi.Context(w, h, frame_slots=B + 2, flow_slots=B, max_batch=B) as ctx:
                recs, dots = _run_bench_batch(ctx, frames, B)
                flows = [ctx.download_flow(j) for j in range(B)]
        finally:
            _capi.set_option("fuse_first", 10000)
        for j in range(B):
            assert np.array_equal(flows[j], orc.farneback(frames[j], frames[j + 1])), (w, h, B, fuse, j)
            _check_reductions_on_own_flow(None, j, recs[j], flows[j])


def test_reference_operating_point_256x256_b256_against_goldens():
    """FF:1057: every frame is resized to 256x256 before pairing -- the reference's real operating point.  One batch
    of 256 pairs (FFL_MAX_BATCH) per launch sequence, replayed from the captured hipGraph: all 256 records and
    scalars against the oracle goldens; the first step is the capture, the later ones are replays."""
    W = H = B = 256
    frames = sine_translate_frames(B + 1, W, H, seed=1)
    gold = golden_check.load_golden(W, H, B, 1)
    assert gold is not None
    with _capi.Context(W, H, frame_slots=B + 2, flow_slots=2 * B, max_batch=B) as ctx:
        ctx.upload_frames(0, list(frames))
        for step in range(3):
            slots = [(step % 2) * B + i for i in range(B)]
            ctx.flow_pairs(list(range(B)), list(range(1, B + 1)), slots)
            recs = ctx.pass1_results(slots, 7.0)
            centers = pipeline.smooth_centers([(r[0], r[1]) for r in recs])
            dots = []
            for s0 in range(0, B, 64):
                dots += ctx.radial(slots[s0:s0 + 64], centers[s0:s0 + 64], [r[4] for r in recs[s0:s0 + 64]], False)
            status, detail = golden_check.check_batch(gold, frames, recs, dots, lambda j: ctx.download_flow(slots[j]))
            _require_golden_match(status, f"step {step}: {detail}")
        dots256 = ctx.radial(slots, centers, [r[4] for r in recs], False)     # pass 2 for 256 pairs in one call
        assert dots256 == dots


def test_graph_replay_equals_eager_launches():
    """ffl_set_option("graph"): the captured-graph path and the eager path give identical bits, over batches of
    different shapes on one context (full batches, a ragged last batch, independent pairs, POV), several replays
    each with different frame / flow slot tables."""
    w, h, B = 160, 120, 6
    fr = sine_translate_frames(40, w, h, seed=14, amp=(2.5, 1.5), period=11, zoom=0.02)
    out = {}
    try:
        for graph in (1, 0):
            _capi.set_option("graph", graph)
            with _capi.Context(w, h, max_batch=B, frame_slots=2 * B + 2, flow_slots=pipeline.min_flow_slots(B)) as ctx:
                eng = pipeline.PairEngine(ctx)
                a = eng.process_chunk(fr)                        # 39 pairs: 6 full batches + a ragged one of 3
                b = eng.process_chunk(fr[:20], pov_mode=True)
                ctx.upload_frames(0, list(fr[:8]))
                ctx.flow_pairs([0, 2, 4, 6], [1, 3, 5, 7], [0, 1, 2, 3])   # independent pairs: 8 unique frames
                c = [ctx.download_flow(j) for j in range(4)]
            out[graph] = (a, b, c)
    finally:
        _capi.set_option("graph", 1)
    for x, y in zip(out[1][:2], out[0][:2]):
        assert np.array_equal(x[0], y[0]) and [tuple(r) for r in x[1]] == [tuple(r) for r in y[1]]
    for j in range(4):
        assert np.array_equal(out[1][2][j], out[0][2][j])
        assert np.array_equal(out[1][2][j], orc.farneback(fr[2 * j], fr[2 * j + 1]))


def test_graph_cache_is_bounded_and_shapes_may_vary_freely():
    """More batch shapes than the per-lane graph cache holds (16): every shape is captured, replayed, evicted and
    re-captured without changing a bit (one lane so that all shapes land in the same cache)."""
    w, h, nmax = 96, 64, 20
    fr = sine_translate_frames(nmax + 1, w, h, seed=3, amp=(2.0, 1.0), period=7)
    want = {}
    try:
        _capi.set_option("lanes", 1)
        for graph in (0, 1):
            _capi.set_option("graph", graph)
            with _capi.Context(w, h, max_batch=nmax, frame_slots=nmax + 2, flow_slots=nmax) as ctx:
                ctx.upload_frames(0, list(fr))
                for rep in range(2):
                    for n in list(range(1, nmax + 1)) + [3, 1, nmax]:
                        ctx.flow_pairs(list(range(n)), list(range(1, n + 1)), list(range(n)))
                        got = (ctx.download_flow(n - 1).tobytes(), tuple(ctx.pass1_result(n - 1)))
                        if graph == 0 and rep == 0:
                            want[n] = got
                        assert got == want[n], (graph, rep, n)
    finally:
        _capi.set_option("graph", 1)
        _capi.set_option("lanes", 2)
    assert np.array_equal(np.frombuffer(want[nmax][0], np.float32).reshape(h, w, 2), orc.farneback(fr[nmax - 1], fr[nmax]))


def test_one_results_call_names_more_batch_events_than_sixteen():
    """ffl_pass1_results waits once per DISTINCT event of the slots it names.  24 one-pair batches on two lanes leave 24
    lane events live (12 per lane, each lane's ring holds 16): one call reads all 24 records, and they equal those of one
    24-pair batch of the same pairs on a second context."""
    w, h, n = 96, 64, 24
    fr = sine_translate_frames(n + 1, w, h, seed=5, amp=(2.0, 1.5), period=9)
    slots = list(range(n))
    recs = []
    try:
        _capi.set_option("lanes", 2)
        for one_pair_batches in (True, False):
            with _capi.Context(w, h, max_batch=n, frame_slots=n + 1, flow_slots=n) as ctx:
                ctx.upload_frames(0, list(fr))
                if one_pair_batches:
                    for j in range(n):
                        ctx.flow_pairs([j], [j + 1], [j])
                else:
                    ctx.flow_pairs(list(range(n)), list(range(1, n + 1)), slots)
                recs.append([tuple(r) for r in ctx.pass1_results(slots, 7.0)])
    finally:
        _capi.set_option("lanes", 2)
    assert recs[0] == recs[1]
    assert (recs[0][7][0], recs[0][7][1]) == orc.max_divergence_np(orc.farneback(fr[7], fr[8]))[:2]


def test_largest_baseline_frame_5760x2880_whole():
    """The largest frame BASELINE names, taken whole (SURVEY App. C "5 whole frame": 16.6 Mpx, 332 MB per 5-plane
    field, 8.3 GB of algorithmic traffic per pair): one pair bit for bit against the oracle, reductions on the
    device's own flow, pass 2 -- the 32-bit plane offsets and the largest grids of every kernel."""
    W, H = 5760, 2880
    fr = sine_translate_frames(2, W, H, seed=2, amp=(5.0, 3.0))
    with _capi.Context(W, H, max_batch=1, frame_slots=2, flow_slots=1) as ctx:
        ctx.submit_pair(0, fr[0], fr[1])
        rec = ctx.pass1_result(0)
        flow = ctx.download_flow(0)
        c = (0.47 * W, 0.55 * H)
        got = ctx.radial([0], [c], [False], False)[0]
    assert np.array_equal(flow, orc.farneback(fr[0], fr[1]))
    _check_reductions_on_own_flow(None, 0, rec, flow)
    want = float(orc.radial_np(flow, c, False, False))
    assert abs(got - want) <= 1e-4 * max(abs(want), 1e-6 * W)
    pr.check_radial(got, flow, c, False)


def test_bench_prints_exactly_one_json_line():
    """the driver's contract: stdout of bench.py is ONE JSON line (native libraries' chatter goes to stderr); `checked`
    is the comparison with the oracle goldens that --full makes"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--full", "--no-extras",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert len(lines) == 1, r.stdout[:2000]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "checked"):
        assert k in d, k
    assert d["steps"] == 2 and d["n_gpus"] == 1 and d["checked"] is True


def test_bench_plain_run_times_and_dumps_only(tmp_path):
    """Without --full the benchmark sets up, warms up, times, dumps and prints, nothing else: the line has the headline
    fields and no result of a check, a CPU baseline or an extra pass.  What it dumps is still the oracle golden's
    workload (records bit for bit), and the time the whole process spends outside its steps (start to exit, less
    (steps + warmup) x ms_per_step) stays under the 30 s a plain run may take there."""
    import json
    import time
    W, H, B, steps, warmup = 256, 256, 64, 2, 1
    d = tmp_path / "plain"
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--width", str(W), "--height", str(H), "--batch", str(B), "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert len(lines) == 1, r.stdout[:2000]
    line = json.loads(lines[0])
    assert line["metric"] == f"{W}x{H} frame-pairs/sec" and line["unit"] == "pairs/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["steps"] == steps and line["warmup"] == warmup
    assert line["ms_per_step"] > 0 and abs(line["value"] - B / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert line["checked"] is None and "--full" in line["check_detail"]
    for k in ("cpu_baseline", "kernel_classes", "pcie_inclusive", "small_image", "large_image"):
        assert k not in line, k
    outside = wall - (steps + warmup) * line["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.2f} s wall, {outside:.2f} s outside its steps")
    assert outside <= 30.0, outside
    a = {p.stem: np.load(p) for p in d.iterdir()}
    gold = golden_check.load_golden(W, H, B, 1)
    assert a["argmax_x"].tolist() == gold["x"] and a["argmax_y"].tolist() == gold["y"]
    assert a["max_divergence"].view(np.uint32).tolist() == gold["val_bits"] and a["cut"].astype(bool).tolist() == gold["cut"]


def test_bench_dump_outputs_repeat_and_match_the_golden(tmp_path):
    """--dump-outputs: two runs with the same arguments write the same arrays (bit for bit), --steps sets the number of
    timed steps, and the dumped records / scalars of the last step are those of the oracle golden of that workload."""
    import json
    W, H, B = 256, 256, 64
    dumps = []
    for run, steps in enumerate((2, 3)):
        d = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "1",
                            "--width", str(W), "--height", str(H), "--batch", str(B), "--full", "--no-extras", "--no-cpu-baseline",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.split("\n") if l.strip()][0])
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["checked"] is True, line["check_detail"]
        assert sum(p.stat().st_size for p in d.iterdir()) <= 64 << 20
        dumps.append({p.stem: np.load(p) for p in d.iterdir()})
    a, b = dumps
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    gold = golden_check.load_golden(W, H, B, 1)          # "checked" above: the run's frames are the golden's
    assert a["argmax_x"].tolist() == gold["x"] and a["argmax_y"].tolist() == gold["y"]
    assert a["max_divergence"].view(np.uint32).tolist() == gold["val_bits"] and a["cut"].astype(bool).tolist() == gold["cut"]
    g = np.asarray(gold["dots"], np.float64)
    assert np.all(np.abs(a["radial"] - g) <= 1e-4 * np.maximum(np.abs(g), np.mean(np.abs(g))))
    # the flow sample holds the device's own flow: pair 0 against the oracle at the sampled pixels
    fr = sine_translate_frames(2, W, H, seed=1)
    pix = a["flow_sample_index"].astype(np.int64)
    assert np.array_equal(a["flow_sample"][0], orc.farneback(fr[0], fr[1]).reshape(-1, 2)[pix])


def test_non_default_options_change_no_bit():
    """tile_order = 1 (tile-major workgroup order), pyr_coarse = 0 (H + V kernel pairs for the coarse pyramid levels),
    copy_threads = 1 / 8 (staging copy split) and blur_min_wgs (automatic strip length of k_blur_solve, from a whole tile
    column per workgroup to one tile) are speed options: records, scalars and the flow field must be identical."""
    from funscript_flow_amd.synth import gray_to_bgr
    w, h, B = 640, 360, 8
    frames = sine_translate_frames(B + 1, w, h, seed=21, amp=(3.0, 2.0), period=7, zoom=0.02)
    bgr = gray_to_bgr(frames)

    def run(**opts):
        try:
            for k, v in opts.items():
                _capi.set_option(k, v)
            with _capi.Context(w, h, max_batch=B, frame_slots=2 * B + 2, flow_slots=pipeline.min_flow_slots(B)) as ctx:
                ctx.upload_frames(0, list(bgr))           # staged BGR upload: exercises the copy pool
                slots = list(range(B))
                ctx.flow_pairs(list(range(B)), list(range(1, B + 1)), slots)
                recs = ctx.pass1_results(slots, 7.0)
                centers = pipeline.smooth_centers([(r[0], r[1]) for r in recs])
                dots = ctx.radial(slots, centers, [r[4] for r in recs], False)
                flow = ctx.download_flow(B // 2)
            return recs, dots, flow
        finally:
            _capi.set_option("tile_order", 0)
            _capi.set_option("pyr_coarse", 1)
            _capi.set_option("copy_threads", 4)
            _capi.set_option("blur_min_wgs", 3500)

    ref = run()
    for opts in ({"tile_order": 1}, {"pyr_coarse": 0}, {"copy_threads": 1}, {"copy_threads": 8}, {"tile_order": 1, "fuse_first": 1},
                 {"blur_min_wgs": 1}, {"blur_min_wgs": 200}, {"blur_min_wgs": 100000}):   # one strip per column ... one tile per workgroup
        try:
            got = run(**opts)
        finally:
            _capi.set_option("fuse_first", 10000)
        assert [tuple(r) for r in got[0]] == [tuple(r) for r in ref[0]], opts
        assert got[1] == ref[1], opts
        assert np.array_equal(got[2], ref[2]), opts


def test_largest_batch_1080p_b256_two_lanes_equals_b32_batches():
    """The largest context the API allows at the headline size: 1080p, FFL_MAX_BATCH = 256 pairs per batch, 257 unique
    frames, two lanes (~ 150 GB of work buffers: the R planes of 512 frames alone are 28 GB, far beyond 32-bit byte
    offsets).  Its 256 records must equal those of the same pairs run as eight 32-pair batches (the configuration the
    goldens pin), three flow fields bit for bit, one of them against the oracle."""
    W, H, B = 1920, 1080, _capi.FFL_MAX_BATCH
    base = sine_translate_frames(33, W, H, seed=1)
    frames = [base[i % 33] for i in range(B + 1)]
    need, pinned = _capi.estimate_bytes(W, H, B + 2, B, B)
    free, total = _capi.device_mem_info(0)
    assert need > 100e9, need                      # this IS the big one
    if need > 0.9 * free:
        pytest.skip(f"needs {need / 1e9:.0f} GB of device memory, {free / 1e9:.0f} GB free")
    try:
        _capi.set_option("lanes", 2)
        with _capi.Context(W, H, frame_slots=B + 2, flow_slots=B, max_batch=B) as ctx:
            ctx.upload_frames(0, frames)
            slots = list(range(B))
            ctx.flow_pairs(list(range(B)), list(range(1, B + 1)), slots)
            big = ctx.pass1_results(slots, 7.0)
            keep = {j: ctx.download_flow(j) for j in (0, 131, 255)}
            free_with_ctx, _ = _capi.device_mem_info(0)
        assert free - free_with_ctx <= need * 1.02 and free - free_with_ctx >= need * 0.9, (free - free_with_ctx, need)
        with _capi.Context(W, H, frame_slots=34, flow_slots=64, max_batch=32) as ctx:
            ctx.upload_frames(0, list(base))
            for s0 in range(0, B, 32):
                f0 = [(s0 + i) % 33 for i in range(32)]
                f1 = [(s0 + i + 1) % 33 for i in range(32)]
                sl = [(s0 // 32 % 2) * 32 + i for i in range(32)]
                ctx.flow_pairs(f0, f1, sl)
                small = ctx.pass1_results(sl, 7.0)
                assert [tuple(r) for r in small] == [tuple(r) for r in big[s0:s0 + 32]], s0
                for j, f in keep.items():
                    if s0 <= j < s0 + 32:
                        assert np.array_equal(ctx.download_flow(sl[j - s0]), f), j
    finally:
        _capi.set_option("lanes", 2)
    assert np.array_equal(keep[131], orc.farneback(frames[131], frames[132]))


def test_create_that_exceeds_device_memory_fails_cleanly_and_leaves_the_device_usable():
    """A context that cannot fit (4K, thousands of resident flow fields) must come back as FFL_ERR_HIP with the failing
    allocation named, free everything it had already allocated, and leave the device usable: the next ffl_create
    succeeds and computes the right flow."""
    W, H = 3840, 2160
    free0, total = _capi.device_mem_info(0)
    slots = int(total * 1.2 // (8 * W * H))                # flow fields worth 120 % of the whole device
    need, _ = _capi.estimate_bytes(W, H, 4, slots, 1)
    assert need > total
    with pytest.raises(_capi.FFLError, match=r"ffl_create failed \(2\).*hipMalloc"):
        _capi.Context(W, H, frame_slots=4, flow_slots=slots, max_batch=1)
    free1, _ = _capi.device_mem_info(0)
    assert free1 >= free0 - (64 << 20), (free0, free1)      # nothing of the failed context is left behind
    fr = sine_translate_frames(2, 320, 180, seed=1)
    with _capi.Context(320, 180, max_batch=1) as ctx:
        ctx.submit_pair(0, fr[0], fr[1])
        assert np.array_equal(ctx.download_flow(0), orc.farneback(fr[0], fr[1]))
    # the reference-shaped chunk API sizes itself against free memory and says what to do instead of failing in hipMalloc
    from funscript_flow_amd import backend
    with pytest.raises(_capi.FFLError, match="lower batch_size"):
        backend._fit_chunk(W, H, slots, 0, 32)
    B, bytes_needed = backend._fit_chunk(1920, 1080, 3000, 0, 32)      # the reference's default chunk (FF:2647) at 1080p
    assert 1 <= B <= 32 and bytes_needed < free1


def test_a_contexts_whole_life_leaves_no_device_memory_behind():
    """Everything a context allocates AFTER ffl_create goes with it: the raw-frame ring (grown once), the descriptor
    tables of the device upload, two captured graphs, the general Farneback work area, the import buffers, a pinned frame
    buffer the caller never frees, the profiling events.  Three contexts in a row, 1080p, max_batch 8: after each close
    the free device memory is back within 64 MiB of where it started (one lane's buffers alone are above 2 GB here, so
    any array left behind shows).  The torch tensors exist before the starting value is read: the caching allocator
    keeps what it once took."""
    import torch
    W, H, B = 1920, 1080, 8
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    small = [rng.integers(0, 256, (H // 2, W // 2, 3), dtype=np.uint8) for _ in range(8)]
    large = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    dev_frames = torch.from_numpy(rng.integers(0, 256, (2, H, W), dtype=np.uint8)).to(dev)
    fields = torch.from_numpy(rng.standard_normal((2, H, W, 2)).astype(np.float32)).to(dev)
    exported = torch.empty((2, H, W, 2), dtype=torch.float32, device=dev)
    general = _capi.FarnebackParams(pyr_scale=0.8, levels=6)
    # 2 x max_batch unique frames: the general path then needs exactly the extra bytes, so its work area IS allocated
    assert _capi.farneback_extra_bytes(W, H, B, general) > 0
    torch.cuda.synchronize(dev)
    free0, _ = _capi.device_mem_info(0)
    for life in range(3):
        with _capi.Context(W, H, max_batch=B) as ctx:
            assert ctx.frame_slots >= 18 and ctx.flow_slots >= 24
            ctx.upload_frames_raw(0, small, (W, H))               # the ring's first buffers ...
            ctx.upload_frames_raw(8, large, (W, H))               # ... and every one of them grown
            ctx.upload_frames_device(16, dev_frames, "gray")
            ctx.flow_pairs(list(range(8)), list(range(1, 9)), list(range(8)))           # two batch shapes: two graphs
            ctx.flow_pairs([0, 1, 2], [1, 2, 3], [8, 9, 10])
            ctx.flow_pairs_farneback(list(range(8)), list(range(8, 16)), list(range(11, 19)), params=general)
            ctx.import_flows(fields, [19, 20])
            ctx.export_flows([0, 1], exported)
            pinned = ctx.pinned_frames(2)                         # never freed by the caller
            pinned[:] = dev_frames.cpu().numpy()
            ctx.upload_frames(16, list(pinned))
            ctx.profile_enable(True)
            ctx.flow_pairs([16], [17], [21])
            assert len(ctx.pass1_results(list(range(22)))) == 22
            ctx.profile_enable(False)
            assert ctx.graph_stats()["capture_failures"] == 0
            free_open, _ = _capi.device_mem_info(0)
            assert free0 - free_open > 2 << 30, (free0, free_open)
            del pinned
        torch.cuda.synchronize(dev)
        free1, _ = _capi.device_mem_info(0)
        assert free1 >= free0 - (64 << 20), (life, free0, free1)


def test_options_belong_to_a_context_not_to_the_process():
    """Two live contexts in one process (the shape of one process driving several GPUs): each keeps the option set it was
    created with, ffl_ctx_set_option changes ONE of them and makes only that one re-capture its graphs, "lanes" is fixed
    at creation, and nothing of it changes a bit of the results."""
    w, h, B = 320, 180, 4
    fr = sine_translate_frames(B + 1, w, h, seed=8, amp=(2.5, 1.5), period=7, zoom=0.02)
    want = [orc.farneback(fr[j], fr[j + 1]) for j in range(B)]

    def step(ctx):
        ctx.flow_pairs(list(range(B)), list(range(1, B + 1)), list(range(B)))
        return [ctx.download_flow(j) for j in range(B)]

    try:
        _capi.set_option("lanes", 1)
        _capi.set_option("fuse_first", 1)
        a = _capi.Context(w, h, frame_slots=B + 2, flow_slots=B, max_batch=B)
        _capi.set_option("lanes", 2)
        _capi.set_option("fuse_first", 10000)          # process-wide defaults changed AFTER a exists: a keeps its own
        b = _capi.Context(w, h, frame_slots=B + 2, flow_slots=B, max_batch=B)
        with a, b:
            assert (a.get_option("lanes"), a.get_option("fuse_first")) == (1, 1)
            assert (b.get_option("lanes"), b.get_option("fuse_first")) == (2, 10000)
            for c in (a, b):
                c.upload_frames(0, list(fr))
                for _ in range(3):
                    for got, w_ in zip(step(c), want):
                        assert np.array_equal(got, w_)
            ga, gb = a.graph_stats(), b.graph_stats()
            assert ga["capture_failures"] == gb["capture_failures"] == 0 and ga["captured"] == 1 and gb["captured"] == 2   # one per lane used
            a.set_option("blur_min_wgs", 1)             # a knob of a alone: a re-captures, b replays what it has
            a.set_option("tile_order", 1)
            assert b.get_option("blur_min_wgs") == 3500 and b.get_option("tile_order") == 0
            assert _capi.get_option("blur_min_wgs") == 3500
            for c in (a, b):
                for _ in range(2):
                    for got, w_ in zip(step(c), want):
                        assert np.array_equal(got, w_)
            ga2, gb2 = a.graph_stats(), b.graph_stats()
            assert ga2["captured"] == ga["captured"] + 1 and gb2["captured"] == gb["captured"], (ga, ga2, gb, gb2)
            assert gb2["replayed"] == gb["replayed"] + 2 and ga2["capture_failures"] == gb2["capture_failures"] == 0
            with pytest.raises(_capi.FFLError):         # a fixed knob: the refusal changes nothing, so a replays its graph
                a.set_option("run_ahead", 1)
            assert a.get_option("run_ahead") == 0
            for got, w_ in zip(step(a), want):
                assert np.array_equal(got, w_)
            ga3 = a.graph_stats()
            assert ga3["captured"] == ga2["captured"] and ga3["replayed"] == ga2["replayed"] + 1, (ga2, ga3)
            with pytest.raises(_capi.FFLError, match="lanes"):
                a.set_option("lanes", 2)
            a.set_option("lanes", 1)                    # the value it has is accepted
            with pytest.raises(_capi.FFLError):
                a.set_option("no_such_knob", 1)
    finally:
        _capi.set_option("lanes", 2)
        _capi.set_option("fuse_first", 10000)


def test_sync_from_another_thread_while_new_batch_shapes_are_captured():
    """ffl_sync must not touch a lane's stream while another thread captures a graph on it (advisor, round 3): one thread
    queues batches of ever new shapes (every one a fresh hipStreamBeginCapture .. EndCapture on the lane's stream), a
    second thread calls ffl_sync in a loop.  No call may fail, no capture may be invalidated, results stay exact."""
    import threading
    w, h, nmax = 160, 96, 12
    fr = sine_translate_frames(nmax + 1, w, h, seed=6, amp=(2.0, 1.0), period=7)
    errors, stop = [], threading.Event()
    try:
        _capi.set_option("lanes", 1)
        with _capi.Context(w, h, max_batch=nmax, frame_slots=nmax + 2, flow_slots=nmax) as ctx:
            ctx.upload_frames(0, list(fr))
            ctx.sync()

            def syncer():
                try:
                    while not stop.is_set():
                        ctx.sync()
                except Exception as e:  # noqa: BLE001
                    errors.append(e)

            t = threading.Thread(target=syncer)
            t.start()
            try:
                for rep in range(3):
                    for n in range(1, nmax + 1):
                        for pov in (False, True):          # 24 shapes per round > the 16-entry cache: captures every round
                            ctx.flow_pairs(list(range(n)), list(range(1, n + 1)), list(range(n)), pov)
            finally:
                stop.set()
                t.join()
            assert not errors, errors
            gs = ctx.graph_stats()
            assert gs["capture_failures"] == 0 and gs["captured"] >= 2 * nmax, gs
            ctx.flow_pairs([nmax - 1], [nmax], [0])
            assert np.array_equal(ctx.download_flow(0), orc.farneback(fr[nmax - 1], fr[nmax]))
    finally:
        _capi.set_option("lanes", 2)


def test_long_chunk_outlives_the_event_rings():
    """A chunk of far more batches than the event rings have entries (16 per lane, 32 upload events), on the frame-ring
    geometry that exposed stale event handles in round 4: 4 (B + 1) frame slots, two lanes -- a slot's last-use reference of
    the OTHER lane then goes more than a ring's length without being refreshed.  A stale reference must count as completed
    (never as "wait for whatever that ring entry stands for now"), and nothing about the order of uploads, batches and pass
    2 may change: the chunk's records and scalars equal those of a one-lane context with ample slots, frames fed from
    page-locked memory (zero-copy uploads) and from ndarrays alike, and sampled pairs equal the oracle."""
    w, h, B, n = 96, 64, 4, 230                                       # 229 pairs = 58 batches: the lanes' rings wrap twice
    base = sine_translate_frames(23, w, h, seed=9, amp=(2.0, 1.5), period=11, zoom=0.02)
    frames = [base[i % 23] for i in range(n)]
    try:
        _capi.set_option("lanes", 1)
        with _capi.Context(w, h, max_batch=B, frame_slots=64, flow_slots=64) as ref_ctx:
            want_dots, want_recs = pipeline.PairEngine(ref_ctx, depth=1).process_chunk(frames)
        _capi.set_option("lanes", 2)
        for pinned in (False, True):
            with _capi.Context(w, h, max_batch=B, frame_slots=4 * (B + 1), flow_slots=pipeline.min_flow_slots(B, 2)) as ctx:
                fl = frames
                if pinned:
                    store = ctx.pinned_frames(n)
                    for i in range(n):
                        store[i] = frames[i]
                    fl = [store[i] for i in range(n)]
                dots, recs = pipeline.PairEngine(ctx, depth=2).process_chunk(fl)
                assert ctx.graph_stats()["capture_failures"] == 0
            assert np.array_equal(dots, want_dots), pinned
            assert [tuple(r) for r in recs] == [tuple(r) for r in want_recs], pinned
    finally:
        _capi.set_option("lanes", 2)
    centers = pipeline.smooth_centers([(r[0], r[1]) for r in want_recs])
    for j in (0, 101, 228):
        flow = orc.farneback(frames[j], frames[j + 1])
        assert (want_recs[j][0], want_recs[j][1]) == orc.max_divergence_np(flow)[:2], j
        ref = float(orc.radial_np(flow, centers[j], want_recs[j][4], False))
        assert abs(want_dots[j] - ref) <= 1e-4 * max(abs(ref), 1e-3), j
        if not want_recs[j][4]:
            pr.check_radial(float(want_dots[j]), flow, centers[j], False)


def test_staged_upload_of_many_frames_with_a_row_stride_is_shared_by_the_copy_threads():
    """ffl_upload_frames stages a run of frames with its rows split over the copy threads (CopyPool::copy), also when the
    frames are views with a row stride (the right halves of wider arrays) and when a thread's share starts in the middle
    of a frame: 37 frames of 300x200 (2.2 MB: above the 1 MiB threshold), 1 / 3 / 4 / 7 copy threads, gray and BGR."""
    w, h, n = 300, 200, 37
    rng = np.random.default_rng(5)
    wide = rng.integers(0, 256, (n, h, 2 * w + 3), dtype=np.uint8)
    views = [wide[i][:, w + 3:] for i in range(n)]                       # row stride 2w + 3, rows not contiguous
    wide3 = rng.integers(0, 256, (n, h, w + 5, 3), dtype=np.uint8)
    views3 = [wide3[i][:, 5:, :] for i in range(n)]
    assert not views[0].flags["C_CONTIGUOUS"] and not views3[0].flags["C_CONTIGUOUS"]
    for threads in (1, 3, 4, 7):
        with _capi.Context(w, h, max_batch=4, frame_slots=n + 1, flow_slots=4) as ctx:
            ctx.set_option("copy_threads", threads)
            ctx.upload_frames(1, views)
            for i in (0, 1, 17, 35, 36):
                assert np.array_equal(ctx.download_frame(1 + i), views[i]), (threads, i)
            ctx.upload_frames(0, views3)
            for i in (0, 9, 36):
                assert np.array_equal(ctx.download_frame(i), orc.bgr2gray(np.ascontiguousarray(views3[i]))), (threads, i)


@pytest.mark.parametrize("assign", ["contiguous", "round_robin"])
def test_bench_one_clip_is_checked_against_the_oracle_golden(assign):
    """`bench.py --one-clip` (strong-scaling form; contiguous = the halo-only streaming exchange): its `checked` must come
    from the oracle golden of the seed-1 stream (records of pairs 0..31, scalars of pairs 0..25), not only from the clip's
    period-16 self-consistency (advisor, round 3)."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--one-clip", "--assign", assign, "--steps", "2", "--no-cpu-baseline"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["mode"] == "one_clip" and line["scaling"] == "strong" and line["n_gpus"] == 1 and line["value"] > 0
    if line["checked"] is None:
        pytest.skip(line["check_detail"])
    assert line["checked"] is True and "oracle golden" in line["check_detail"], line["check_detail"]
