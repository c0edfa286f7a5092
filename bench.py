"""bench.py -- the BASELINE.json metric on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, runs W warm-up steps, times K steps and prints the headline line (`metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step`, ...) and nothing else.  `--dump-outputs DIR` writes what the last timed step
returned as float32 .npy files (see dump_outputs).  `--full` adds everything beyond the headline: the objects listed below,
the parity check against the reference's own run and the host-enqueue diagnostic (`--no-*` switch single legs off).

N > 1: one process per GPU over RCCL (torch.distributed backend "nccl").  Started as the driver starts it
(`python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...`) the ranks read
RANK / LOCAL_RANK / WORLD_SIZE from the environment; started as plain `python bench.py --gpus N` with no WORLD_SIZE
set, this file re-executes itself under torch.distributed.run with N ranks on 127.0.0.1 -- either way
`n_gpus` in the JSON line is the number of ranks that really ran, and `--gpus` must equal it.

One "step" = one pass of the per-clip inference hot path over one synthetic clip per rank:
  BASELINE config 2 -- Swin-T UniVS, T=5 frames @ 720p (zero-padded to 736x1280), 100 learnable queries,
  first clip of a video (no prompt queries): normalise+pad -> Swin-T -> MSDeformAttn pixel decoder ->
  UniVS decoder (9 layers, 10 prediction heads) -> pred_masks [1,100,5,184,320].
Inputs (frames, closed-form weights) are resident in HBM before the timed region.  fp32 end to end (the
parity contract is 1e-3 max-abs on mask logits against the reference's fp32 CPU path).

`value` (headline): clip replicas -- each rank runs its own clip (clips of different videos are independent: SURVEY.md
section 8e, no data-path collective), weak scaling, whole-job frames/s.
`frame_sharded` (N > 1 only, BASELINE config 3): ONE clip of 5*N frames (T=40 at N=8) sharded by frame: backbone, pixel
decoder, cross-attention, FFN and mask decode on the local frames, one RCCL all-gather of the query states per decoder
layer (univs_amd/distributed.py) -- measured right after the replica loop in the same processes.

Nothing is measured inside the timed region except the steps themselves: per-kernel times for the roofline objects
come from a separate instrumented pass after it (HIP events on the launch stream around each operator call).

Extra objects on the JSON line with `--full` (tier contract): `roofline` (MSDeformAttn forward, algorithmic bytes 3200*S per frame
per launch), `roofline_mask_decode` (the full-resolution launch) and `roofline_mask_decode_family`
(the ten prediction-head calls of a clip under the un-fused op-boundary accounting of SURVEY.md section 8d: 4.197 GB per
clip over the summed time of every kernel the fused implementation runs for them), `roofline_window_attn` (per Swin
stage), and `cpu_baseline` (rank 0, N=1 only: the CPU oracle path on the host cores, 1 warm-up + 3 timed clips, median).
Informational objects (never `value`): `steady_state_with_prompts` (second clip of a video, 10 entities), `config4_swinb_refvos`
(BASELINE config 4: Swin-B, 200 queries + 4 referring expressions), `config5_swinl_1080p`, `frame_sharded_n1` (one 40-frame clip under a
one-rank RCCL group) and `sliding_clip_loop` (config 3 as the reference RUNS a long video: the sliding 5-frame clip loop with the prompt
memory pool over a 20-frame video -- at N = 1 in the reference's call pattern and in this build's default; at N > 1 with the frames of
the video spread over the N ranks, InferenceVideoEntity.set_frame_shard).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

# dmabuf IPC: RCCL (and CUDA-tensor sharing across processes) needs it on this host driver.  Set before the HIP / HSA runtime
# can initialise -- i.e. before `import torch` -- so that it holds however the ranks were started (the driver's
# `python -m torch.distributed.run ... bench.py`, our own relaunch, or a single process).
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # B/s, MI355X_MICROARCH.md "HBM3E peak BW" (spec)
F32_MFMA_PEAK = 157.3e12   # FLOP/s, MI355X_MICROARCH.md "Peak FP32 (matrix)"


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned to DIR/<name>.npy (float32; rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement and check beyond the headline (other configs, sliding loop, rooflines, "
                         "parity against golden g12, cpu_baseline)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the cpu_baseline leg (default: min(cores, 32))")
    ap.add_argument("--no-frame-sharded", action="store_true", help="skip the config-3 frame-sharded measurement (N>1: one clip "
                    "of 5*N frames over the ranks; N=1: the 40-frame anchor under a one-rank RCCL group)")
    ap.add_argument("--no-config5", action="store_true", help="skip the config-5 (Swin-L, 1080p) clip measurement at N = 1")
    ap.add_argument("--no-sliding-loop", action="store_true", help="skip the sliding-clip-loop video measurement (config 3 as the reference runs it)")
    ap.add_argument("--no-config4", action="store_true", help="skip the config-4 (Swin-B, 200 queries + text prompts) clip measurement at N = 1")
    ap.add_argument("--dry-run", action="store_true",
                    help="CPU / gloo plumbing check (tests): launcher, rendezvous, barrier-bracketed timing, max over "
                         "ranks, JSON line -- with a trivial step instead of the model")
    return ap.parse_args(argv)


def relaunch_under_torchrun(args):
    """`python bench.py --gpus N` with N > 1 and no rendezvous environment: start N ranks ourselves."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL needs it on this driver
    return subprocess.call(cmd, env=env)


def init_distributed(args):
    """-> (world, rank, local_rank).  Asserts that the number of ranks is what --gpus asked for."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a {world}-GPU run as "
                         f"{args.gpus} GPUs")
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # (see the top of the file; kept here for callers that import this function)
        # one process per GPU on one node: share the host cores instead of N x all-cores thread pools
        torch.set_num_threads(max(1, (os.cpu_count() or world) // world))
        if args.dry_run:
            dist.init_process_group("gloo")
        elif os.environ.get("UNIVS_BENCH_ONE_GPU_DEBUG") == "1":
            # DEVELOPMENT ONLY (never set by the driver): all N ranks on GPU 0 with gloo collectives on device tensors -- the N > 1 code
            # paths (replicas, frame_sharded, the sharded sliding loop with its teams) run end to end on the one-GPU boxes; the times mean nothing
            local_rank = 0
            torch.cuda.set_device(0)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    return world, rank, local_rank


def timed_loop(step, steps, warmup, world, sync, dev):
    """W untimed steps, then exactly K steps bracketed by barrier + device sync on both sides; max over ranks."""
    import torch.distributed as dist
    out = None
    for _ in range(warmup):
        out = step()
    sync()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    sync()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt, out


DUMP_MAX_ELEMENTS = 1 << 23        # per array: 32 MB of float32; the config-2 line writes 35.6 MB in all
DUMP_SEED = 0


def dump_outputs(out, path):
    """--dump-outputs: every floating-point tensor of the step's output dict as `path/<key>.npy` (float32).  An array of more
    than DUMP_MAX_ELEMENTS elements (pred_masks: [1, 100, 5, 184, 320] = 118 MB at config 2) is written as `<key>_sample.npy`:
    the elements at DUMP_MAX_ELEMENTS flat indices drawn without replacement by numpy.random.default_rng(DUMP_SEED), ascending --
    the same indices in every run of the same shape."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    total = 0
    for k, v in out.items():
        if not isinstance(v, torch.Tensor) or not v.is_floating_point():
            continue
        v, name = v.detach(), k
        if v.numel() > DUMP_MAX_ELEMENTS:
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(v.numel(), DUMP_MAX_ELEMENTS, replace=False))
            v, name = v.reshape(-1)[torch.from_numpy(idx).to(v.device)], k + "_sample"
        a = v.float().cpu().numpy()
        total += a.nbytes
        assert total <= 64 << 20, f"--dump-outputs: {total} bytes is over the 64 MB budget"
        np.save(os.path.join(path, name + ".npy"), a)


class OpTimer:
    """HIP events (torch.cuda.Event on torch's current stream, which is the stream the C ABI is handed) around every
    call of one `univs_amd.ops` function, keyed by a caller-supplied classification of its arguments."""

    def __init__(self, module, name, key=lambda *a, **k: "all", after=None, keep_args=0):
        self.module, self.name, self.orig = module, name, getattr(module, name)
        self.events, self.enabled, self.key, self.after = {}, False, key, after
        self.notes = {}
        self.keep_args, self.args = keep_args, []        # the first `keep_args` calls' arguments (for replay())

        def wrapped(*a, **k):
            if not self.enabled:
                return self.orig(*a, **k)
            kk = self.key(*a, **k)
            if len(self.args) < self.keep_args:
                self.args.append((a, k))
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = self.orig(*a, **k)
            e.record()
            self.events.setdefault(kk, []).append((s, e))
            if self.after is not None:
                self.notes.setdefault(kk, []).append(self.after())
            return out
        setattr(module, name, wrapped)

    def seconds(self, kk="all"):
        """(average seconds per call, calls) for one class"""
        ev = self.events.get(kk)
        if not ev:
            return None, 0
        return sum(s.elapsed_time(e) for s, e in ev) / len(ev) * 1e-3, len(ev)

    def replay(self, repeats=10):
        """Average seconds per launch with the kept calls' real operands launched back to back, `repeats` times each,
        between ONE pair of HIP events per call (an event pair around every single launch adds ~7 us of record overhead
        to a 170-us kernel; rocprofv3's kernel trace of the same command agrees with this number)."""
        tot, n = 0.0, 0
        for a, k in self.args:
            for _ in range(2):
                self.orig(*a, **k)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(repeats):
                self.orig(*a, **k)
            e.record()
            e.synchronize()
            tot += s.elapsed_time(e) * 1e-3
            n += repeats
        return (tot / n, n) if n else (None, 0)

    def total_seconds(self, pred=lambda kk: True):
        return sum(s.elapsed_time(e) for kk, ev in self.events.items() if pred(kk) for s, e in ev) * 1e-3


def op_rooflines(ops, run_clip, sync, T, S, Qp, C, H, W, passes=2):
    """HBM rooflines of the two north-star operators inside ANOTHER config's clip (BASELINE configs 4 and 5: other S, other Q'):
    HIP events around every msda_forward_heads / mask_decode call of `passes` extra clips (untimed region), net of an empty event
    pair's own cost.  Algorithmic bytes as SURVEY.md 8d defines them: 3200 S T per MSDA launch, 4 (C HW + Q' C + Q' HW) T per
    full-resolution mask decode."""
    tm = OpTimer(ops, "msda_forward_heads", after=ops.msda_last_tiled_generation)
    td = OpTimer(ops, "mask_decode", after=ops.mask_decode_last_impl)
    try:
        tm.enabled = td.enabled = True
        for _ in range(passes):
            run_clip()
        sync()
    finally:
        tm.enabled = td.enabled = False
        setattr(ops, tm.name, tm.orig)
        setattr(ops, td.name, td.orig)
    pairs = []
    for _ in range(100):
        s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        e0.record()
        pairs.append((s0, e0))
    sync()
    ovh = sorted(a_.elapsed_time(b_) for a_, b_ in pairs)[len(pairs) // 2] * 1e-3
    out = {}
    sec, n = tm.seconds()
    if n and set(tm.notes.get("all", [])) == {6}:
        alg, net = 3200.0 * S * T, max(sec - ovh, 0.5 * sec)
        out["roofline"] = {"kernel": "msda_fwd_heads<3> (generation 6) + fused msda_prepare", "bound": "hbm", "achieved": alg / net / 1e9,
                           "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": alg / net / HBM_PEAK, "traffic": None,
                           "avg_launch_us": net * 1e6, "event_pair_us": sec * 1e6, "launches_per_step": n // passes,
                           "algorithmic_bytes_per_launch": alg, "tokens_per_frame": S, "frames": T}
    sec, n = td.seconds()
    if n:
        alg, net = 4.0 * (C * H * W + Qp * C + Qp * H * W) * T, max(sec - ovh, 0.5 * sec)
        out["roofline_mask_decode"] = {"kernel": "skinny_gemm_bf16x6_n32 (full-resolution mask decode; more than 106 query rows run as "
                                                 "balanced row passes over the same columns)", "bound": "hbm",
                                       "achieved": alg / net / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": alg / net / HBM_PEAK,
                                       "traffic": None, "avg_launch_us": net * 1e6, "event_pair_us": sec * 1e6,
                                       "launches_per_step": n // passes, "algorithmic_bytes_per_launch": alg, "queries": Qp,
                                       "impl": sorted(set(td.notes.get("all", [])))}
    return out


def cpu_model_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def dry_run(args, world, rank):
    import torch.distributed as dist
    a = torch.randn(64, 64)

    def step():
        return a @ a

    dt, _ = timed_loop(step, args.steps, args.warmup, world, lambda: None, torch.device("cpu"))
    line = None
    if rank == 0:
        line = json.dumps({"metric": "dry-run (launcher / rendezvous / timing plumbing only)", "value": world * args.steps / dt,
                           "unit": "steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                           "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
                           "backend": dist.get_backend() if world > 1 else "none", "data": "synthetic"})
    if world > 1:
        dist.destroy_process_group()
    return line


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(relaunch_under_torchrun(args))
    # stdout carries the ONE JSON line and nothing else: libraries that write to file descriptor 1 on their own (RCCL's
    # version banner at communicator creation, hipcc when the library is rebuilt on first use) are sent to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    try:
        line = run(args)
    finally:
        sys.stdout.flush()
        ctypes.CDLL(None).fflush(None)         # C stdio buffers too (RCCL prints its banner with printf)
        os.dup2(json_fd, 1)
        os.close(json_fd)
    if line is not None:
        print(line, flush=True)


def run(args):
    world, rank, local_rank = init_distributed(args)
    if args.dry_run:
        return dry_run(args, world, rank)
    import torch.distributed as dist
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP extension is the only implementation)"
    dev = torch.device("cuda", local_rank)

    import __graft_entry__
    if rank == 0:
        __graft_entry__.build()
    if world > 1:
        dist.barrier()
    from univs_amd import ops, runtime, synth
    from univs_amd import workloads as cases
    helpers = cases                                           # model factories live in univs_amd/workloads.py

    gemm_note = runtime.enable_tuned_gemms()      # hipBLASLt / rocBLAS algorithm table (fp32 unchanged)
    swin = helpers.build_swin(dev)
    head = helpers.build_head(cases.CFG2, dev, return_aux=False)
    case = cases.CFG2
    frames = cases.cfg2_frames().to(dev)                      # [5,3,720,1280], 0..255
    mean = torch.tensor([123.675, 116.28, 103.53], device=dev).view(1, 3, 1, 1)
    std = torch.tensor([58.395, 57.12, 57.375], device=dev).view(1, 3, 1, 1)
    T, Q = case["T"], case["Q"]

    def targets(frame_indices=None):
        # (frame indices stay on the host, as the clip loops hand them over: inference_video_entity.py:307 `torch.arange(i, ...)`)
        tv = {k: (v.to(dev) if isinstance(v, torch.Tensor) and k != "frame_indices" else v) for k, v in cases.targets_first_clip(case)[0].items()}
        if frame_indices is not None:
            tv["frame_indices"] = frame_indices
        return [tv]

    @torch.no_grad()
    def step():
        # normalise + pad (720 -> 736 rows): the drivers' pre-step (inference/video_entity.py: normalized_image_list), one pass
        x = ops.normalize_pad(frames, mean, std, pad_to=(736, 1280))
        if x is None:
            x = torch.nn.functional.pad((frames - mean) / std, (0, 0, 0, 16))
        return head(swin(x), targets=targets())

    sync = torch.cuda.synchronize
    dt, out = timed_loop(step, args.steps, args.warmup, world, sync, dev)
    if args.dump_outputs and rank == 0:
        dump_outputs(out, args.dump_outputs)

    res = {
        "metric": "frames/sec per node, 720p T=5 clip, Swin-T 100Q; mask-logit max-abs-err",
        "value": world * T * args.steps / dt,
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "arithmetic": "fp32 I/O and fp32 accumulation everywhere; Linears / MLPs / 1x1 and 3x3 convolutions / 7x7 window attention / the "
                      "decoder's attention (scores and P V) and per-token Linears multiply on the fp16 matrix cores as THREE products of "
                      "two-part fp16 splits (f16x3: ~22-bit effective mantissa, error <= 2^-21.7 per product); mask decode as six bf16 "
                      "products (bf16x6); the decoder FFN's second Linear and the class head in the library's fp32",
        "data": "synthetic",
        "config": {"workload": "BASELINE config 2: Swin-T UniVS, T=5 @ 720p (736x1280 padded), 100 queries, "
                               "first clip (no prompt queries); one clip per GPU",
                   "frames_per_clip": T, "queries": Q, "parallelism": f"clip-replicas x{world}"},
        "gemm_algorithms": gemm_note,
    }
    if world > 1:
        res["rccl"] = {"ranks": dist.get_world_size(), "backend": dist.get_backend(),
                       "version": ".".join(str(v) for v in torch.cuda.nccl.version())}

    if args.full:
        # diagnostic, outside the timed region: how long the host needs to ENQUEUE a clip (python + launch overhead + any
        # host-device synchronisation inside the model).  Close to ms_per_step = the clip is host-bound, not GPU-bound.
        sync()
        t_enq = []
        for _ in range(3):
            t0 = time.perf_counter()
            step()
            t_enq.append(time.perf_counter() - t0)
            sync()
        res["host_enqueue_ms_per_step"] = sorted(t_enq)[1] * 1e3

    # ---- BASELINE config 3: one clip of 5*N frames sharded by frame over the N ranks (T=40 at N=8)
    if args.full and world > 1 and not args.no_frame_sharded:
        from univs_amd.distributed import FrameShard
        head.predictor.frame_shard = FrameShard()
        fr_s = synth.synthetic_frames(T, case["H"], case["W"], f"frames/rank{rank}").to(dev)
        fidx = torch.arange(T * world, device=dev)

        @torch.no_grad()
        def step_sharded():
            x = torch.nn.functional.pad((fr_s - mean) / std, (0, 0, 0, 16))
            return head(swin(x), targets=targets(fidx))

        steps_s = max(3, args.steps // 2)
        try:       # (a failure here -- the same on every rank -- must not cost the replica headline above)
            dts, _ = timed_loop(step_sharded, steps_s, min(args.warmup, 2), world, sync, dev)
            res["frame_sharded"] = {
                "workload": f"BASELINE config 3: ONE clip of {T * world} frames @ 720p, {T} frames per GPU, RCCL all-gather of "
                            "the query states per decoder layer (all_gather_into_tensor)",
                "value": T * world * steps_s / dts, "unit": "frames/s", "frames_per_clip": T * world, "steps": steps_s,
                "ms_per_step": dts / steps_s * 1e3, "scaling": "weak"}
        except Exception as e:  # pragma: no cover
            res["frame_sharded"] = {"error": repr(e)[:300]}
        finally:
            head.predictor.frame_shard = None

    # ---- N = 1 anchor of the frame-sharded path: ONE 40-frame 720p clip (config 3's single-clip reading: position_encoding.py:123
    # allows 128 frames) through FrameShard under a ONE-rank RCCL group, collectives issued for real -- the denominator a
    # later 8-GPU number of `frame_sharded` needs, and the sharded code path on hardware at all
    if args.full and world == 1 and not args.no_frame_sharded:
        try:
            import socket
            from univs_amd.distributed import FrameShard
            with socket.socket() as s_:
                s_.bind(("127.0.0.1", 0))
                port = s_.getsockname()[1]
            dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                    device_id=torch.device("cuda", local_rank))
            T40 = 40
            head.predictor.frame_shard = FrameShard(always_collective=True)
            fr40 = synth.synthetic_frames(T40, case["H"], case["W"], "frames/t40").to(dev)
            fidx40 = torch.arange(T40, device=dev)
            sa_events = []
            hooks = []
            for layer in head.predictor.transformer_self_attention_layers:
                def pre(m, a, k=None, _e=sa_events):
                    e0 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _e.append([e0, None])

                def post(m, a, o, _e=sa_events):
                    e1 = torch.cuda.Event(enable_timing=True)
                    e1.record()
                    _e[-1][1] = e1
                hooks += [layer.register_forward_pre_hook(pre), layer.register_forward_hook(post)]

            @torch.no_grad()
            def step40():
                x40 = torch.nn.functional.pad((fr40 - mean) / std, (0, 0, 0, 16))
                return head(swin(x40), targets=targets(fidx40))
            for _ in range(2):            # the first clip of this length grows the allocator (17 GB) and opens the RCCL channels
                step40()
            sync()
            torch.cuda.reset_peak_memory_stats(dev)
            sa_events.clear()
            t0 = time.perf_counter()
            for _ in range(3):
                o40 = step40()
            sync()
            dt40 = (time.perf_counter() - t0) / 3
            sa_ms = sum(a_.elapsed_time(b_) for a_, b_ in sa_events) / 3
            for h_ in hooks:
                h_.remove()
            head.predictor.frame_shard = None
            # what ONE of 8 ranks evaluates of that self-attention in frame-sharded mode (univs_decoder.py: the query rows of
            # its own 5 frames against the keys of all 40): timed directly on tensors of those shapes, all decoder layers
            Qp = int(o40["pred_masks"].shape[1])
            t_loc, n8 = T40 // 8, 8
            kv_ = synth.normal("bench/sa_rows/kv", (Qp * T40, 1, 256)).to(dev)
            kvp_ = synth.normal("bench/sa_rows/kvp", (Qp * T40, 1, 256)).to(dev)
            rows_ = kv_.view(Qp, T40, 1, 256)[:, :t_loc].reshape(Qp * t_loc, 1, 256).contiguous()
            rowsp_ = kvp_.view(Qp, T40, 1, 256)[:, :t_loc].reshape(Qp * t_loc, 1, 256).contiguous()
            sam_ = head.predictor.generate_self_attn_mask(1, T40, Qp, dev, "ytvis_2021_dev", "detection")
            rmask_ = None if sam_ is None else head.predictor._sa_mask_rows(sam_, Qp, T40, slice(0, t_loc))

            @torch.no_grad()
            def sa_rows():
                for layer in head.predictor.transformer_self_attention_layers:
                    layer(rows_, tgt_mask=rmask_, query_pos=rowsp_, kv=kv_, kv_pos=kvp_)
            for _ in range(2):
                sa_rows()
            ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ea.record()
            for _ in range(3):
                sa_rows()
            eb.record()
            sync()
            sa_rows_ms = ea.elapsed_time(eb) / 3
            per_frame_ms = dt40 * 1e3 - sa_ms           # everything that is per frame (and the one-rank collectives)
            proj_ms = per_frame_ms / n8 + sa_rows_ms
            res["frame_sharded_n1"] = {
                "self_attention_rows_ms_per_clip_at_5_of_40_frames": sa_rows_ms,
                "projected_8_gpus": {"note": "PROJECTION from the N = 1 pieces, not a measurement: (clip - self-attention) / 8 + the "
                                             "row-sharded self-attention of one rank; inter-GPU collective latency (9 all-gathers of "
                                             "0.5 MB + 2 all-reduces per clip) is NOT included",
                                     "ms_per_clip": proj_ms, "speedup": dt40 * 1e3 / proj_ms,
                                     "speedup_if_self_attention_were_replicated": dt40 * 1e3 / (per_frame_ms / n8 + sa_ms)},
                "workload": "ONE clip of 40 frames @ 720p on ONE GPU through FrameShard(world=1) under a one-rank RCCL group "
                            "(all_gather_into_tensor / all_reduce issued per decoder layer)",
                "ms_per_clip": dt40 * 1e3, "frames_per_s": T40 / dt40, "frames_per_clip": T40,
                "peak_memory_gb": torch.cuda.max_memory_allocated(dev) / 2 ** 30,
                "self_attention_ms_per_clip": sa_ms, "self_attention_share": sa_ms / (dt40 * 1e3),
                "self_attention_tokens": int(o40["pred_masks"].shape[1]) * T40,
                "rccl": {"ranks": dist.get_world_size(), "backend": dist.get_backend(),
                         "version": ".".join(str(v) for v in torch.cuda.nccl.version())}}
            del o40, fr40
            dist.destroy_process_group()
            torch.cuda.empty_cache()
        except Exception as e:  # pragma: no cover
            res["frame_sharded_n1"] = {"error": repr(e)[:300]}
            head.predictor.frame_shard = None

    # ---- BASELINE config 5 (Swin-L, T=10 @ 1080p, 200 queries, "MFMA window-attn, fp16"): one clip with the window-attention
    # products on fp16 operands (the variant the config names) and one with the exact-f32 products, on rank 0 at N = 1
    if args.full and world == 1 and not args.no_config5:
        try:
            c5 = cases.CFG5
            swin5 = helpers.build_swin(dev, variant=cases.SWIN_L)
            head5 = helpers.build_head(c5, dev, return_aux=False)
            fr5 = cases.cfg5_frames(c5["T"]).to(dev)
            tg5 = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in cases.targets_first_clip(c5)[0].items()}
            wa = OpTimer(ops, "window_attention_image")

            @torch.no_grad()
            def step5():
                x5 = torch.nn.functional.pad((fr5 - mean) / std, (0, 0, 0, 8))     # 1080 -> 1088 rows
                return head5(swin5(x5), targets=[dict(tg5)])
            c5res = {"workload": "BASELINE config 5: Swin-L (12 x 12 windows), T=10 @ 1080p (1088x1920 padded), 200 queries, "
                                 "first clip; 2 warm-up + 3 timed clips per variant", "frames_per_clip": c5["T"]}
            for mma in ("f16", "f16x3", "f32"):       # fp16 operands (what config 5 names) / fp32-accurate three-product (the default) / exact f32
                swin5.set_attention_mma(mma)
                for _ in range(2):
                    step5()
                sync()
                t0 = time.perf_counter()
                for _ in range(3):
                    step5()
                sync()
                dt5 = (time.perf_counter() - t0) / 3
                wa.enabled = True
                step5()
                sync()
                wa.enabled = False
                c5res[f"window_attention_{mma}"] = {"ms_per_clip": dt5 * 1e3, "frames_per_s": c5["T"] / dt5,
                                                    "window_attention_ms_per_clip": wa.total_seconds() * 1e3,
                                                    "window_attention_launches": sum(len(v) for v in wa.events.values())}
                wa.events.clear()
            setattr(ops, "window_attention_image", wa.orig)
            swin5.set_attention_mma("f16x3")
            c5res.update(op_rooflines(ops, step5, sync, c5["T"], 34 * 60 + 68 * 120 + 136 * 240, c5["Q"], 256, 272, 480))
            res["config5_swinl_1080p"] = c5res
            del swin5, head5, fr5
            torch.cuda.empty_cache()
        except Exception as e:  # pragma: no cover
            res["config5_swinl_1080p"] = {"error": repr(e)[:300]}
            if "wa" in locals():
                setattr(ops, "window_attention_image", wa.orig)

    # ---- BASELINE config 3 as the reference RUNS a long video (inference_video_entity.py:296-316): the sliding 5-frame clip loop with
    # the prompt memory pool carried from clip to clip, over a 20-frame 720p video at the reference's default stride 1 (16 clips).
    #   N = 1: (a) the reference's call pattern (window 5: backbone and pixel decoder once per CLIP), (b) one 20-frame window with the
    #          pixel decoder once per FRAME (inference/video_entity.py: pixel_decoder_once_per_window);
    #   N > 1: the frames of the video spread over the N ranks (frame f on rank f % N: InferenceVideoEntity.set_frame_shard), every
    #          clip's decoder on the ranks that own its frames with one all-gather of the query states per layer, per-video state replicated.
    if args.full and not args.no_sliding_loop:
        try:
            import types
            from univs_amd.inference.video_entity import InferenceVideoEntity, normalized_image_list
            NF = 20
            vid = synth.synthetic_frames(NF, case["H"], case["W"], "cfg3/frames").to(dev)
            model_ns = types.SimpleNamespace(backbone=swin, sem_seg_head=head)

            def make_loop(window):
                return InferenceVideoEntity(
                    hidden_dim=256, num_queries=Q, overlap_threshold_entity=0.5, stability_score_thresh=0.5, size_divisibility=32,
                    pixel_mean=synth.PIXEL_MEAN, pixel_std=synth.PIXEL_STD, num_frames=T, test_topk_per_image=100, apply_cls_thres=0.25,
                    box_nms_thresh=0.85, num_frames_window_test=window, clip_stride=1, num_prev_frames_memory=5,
                    video_unified_inference_entities="", temporal_consistency_threshold=0.25, detect_newly_object_threshold=0.1,
                    detect_newly_interval_frames=1, custom_videos_enable=False).to(dev)

            def run_video(loop):
                torch.manual_seed(0)             # the prompt sampler's draws: the same on every rank
                images = normalized_image_list(list(vid), loop.pixel_mean, loop.pixel_std, 32)
                tg = [{"task": "detection", "dataset_name": "ytvis_2021_dev", "prompt_type": "visual", "num_frames": T,
                       "video_len": NF, "sub_task": "vis"}]
                with torch.no_grad():
                    out = loop.inference_video(model_ns, [{"video_len": NF, "height": case["H"], "width": case["W"]}], images, tg,
                                               merge_results=False)
                n_ent = int(tg[0]["ids"].shape[0]) if "ids" in tg[0] else 0
                return out, n_ent

            def time_video(loop, reps=2):
                run_video(loop)
                sync()
                t0 = time.perf_counter()
                for _ in range(reps):
                    _, n_ent = run_video(loop)
                sync()
                return (time.perf_counter() - t0) / reps, n_ent
            sl = {"workload": f"BASELINE config 3 as the reference runs it: {NF}-frame 720p video, sliding {T}-frame clips at stride 1 "
                              f"({NF - T + 1} clips), visual-prompt memory pool carried between clips; 1 warm-up + 2 timed videos"}
            enc_ = head.predictor.visual_prompt_sampler.visual_prompt_encoder
            sl["sampler_default"] = enc_.sampler_rng

            def with_sampler(mode, loop):
                old_mode = enc_.sampler_rng
                enc_.sampler_rng = mode
                try:
                    return time_video(loop)
                finally:
                    enc_.sampler_rng = old_mode
            if world == 1:
                lp = make_loop(T)
                lp.pixel_decoder_once_per_window = False
                dt_ref, n_ent = with_sampler("reference", lp)
                sl["reference_call_pattern"] = {"window": T, "sampler": "reference", "ms_per_video": dt_ref * 1e3, "frames_per_s": NF / dt_ref,
                                                "entities_at_end": n_ent,
                                                "note": "the reference's algorithm call for call: backbone + pixel decoder once per clip (window = "
                                                        "clip, :309-316), prompt pixels drawn by host-side randperm over every entity's candidates"}
                lp = make_loop(NF)
                dt_w, n_ent = with_sampler("reference", lp)
                sl["one_window_reference_sampler"] = {"window": NF, "sampler": "reference", "ms_per_video": dt_w * 1e3, "frames_per_s": NF / dt_w,
                                                      "entities_at_end": n_ent,
                                                      "note": "backbone and pixel decoder once per frame of the window, decoder per clip"}
                # the library default on the GPU: the prompt sampler draws on the device (same distributions, another random stream, no host
                # round trip, no host randperm over an entity's candidate pixels -- 4 ms each for a large mask at 720p)
                dt_d, n_ent = with_sampler("device", lp)
                sl["one_window"] = {"window": NF, "sampler": "device", "ms_per_video": dt_d * 1e3, "frames_per_s": NF / dt_d, "entities_at_end": n_ent,
                                    "note": "the default configuration of this build (UNIVS_SAMPLER unset: 'auto' = device draws on the GPU)"}
            else:
                from univs_amd.distributed import FrameShard
                team = world                       # (more ranks than a clip has frames: every clip's decoder on the ranks that own its frames)
                import datetime
                # a group of its own with a short timeout: a failure on one rank must not hang the others for the default ten minutes
                grp = dist.new_group(ranks=list(range(team)), timeout=datetime.timedelta(seconds=180))
                dts, failure = 0.0, None
                if rank < team:
                    try:         # (a failing rank still reaches the world-wide reduction below: nobody waits for it in vain)
                        lp = make_loop(NF)
                        fs_loop = FrameShard(group=grp)
                        fs_loop.timeout = datetime.timedelta(seconds=180)        # its sub-groups (one per team of clip owners) too
                        lp.set_frame_shard(fs_loop)
                        lp.replicate_clip_masks = os.environ.get("UNIVS_REPLICATE_CLIP_MASKS") == "1"   # (measurement of the old form only)
                        dts, n_ent = time_video(lp)
                        sl["entities_at_end"] = n_ent
                    except Exception as e_:  # pragma: no cover
                        failure, dts = e_, float("inf")
                tt = torch.tensor([dts], device=dev, dtype=torch.float64)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                dts = float(tt.item())
                if failure is not None:
                    raise failure
                if dts == float("inf"):
                    raise RuntimeError("the frame-sharded sliding clip loop failed on another rank")
                sl["frame_sharded"] = {"ranks_used": team, "ranks_idle": world - team, "window": NF, "ms_per_video": dts * 1e3,
                                       "frames_per_s": NF / dts,
                                       "note": "frame f on rank f % N: backbone + pixel decoder on owned frames, every clip's decoder on the "
                                               "ranks that own one of its frames (ClipShard on a sub-group when N > num_frames), targets[0] "
                                               "replicated; the clip's mask logits stay on the ranks of their frames (ClipMaskRows: per-plane "
                                               "statistics of all rows, the logits of the rows that enter targets[0], candidates' IoU by a maximum)"}
                if rank == 0 and "fs_loop" in locals():
                    clips_ = 3 * (NF - T + 1)                                    # 1 warm-up + 2 timed videos
                    sl["frame_sharded"]["bytes_received_rank0"] = {k_: int(v_) for k_, v_ in fs_loop.bytes.items()}
                    sl["frame_sharded"]["bytes_received_rank0_per_clip"] = {k_: int(v_) // clips_ for k_, v_ in fs_loop.bytes.items()}
                    sl["frame_sharded"]["bytes_per_clip_if_every_row_were_replicated"] = int(4 * (case["Q"] + int(n_ent)) * T * (case["H"] // 4 + 4) * (case["W"] // 4))
            res["sliding_clip_loop"] = sl
        except Exception as e:  # pragma: no cover
            import traceback
            res["sliding_clip_loop"] = {"error": "".join(traceback.format_exception(type(e), e, e.__traceback__))[-600:]}

    # ---- BASELINE config 4: Swin-B (12 x 12 windows), T=5 @ 720p, 200 learnable queries + 4 referring expressions: the text-prompt
    # path (78 text tokens per expression cross-attend to the three feature levels, ...decoder_univs.py:760-793; ProCA; 'sep-blocked'
    # self-attention).  Parity at this size: tests/test_modules_gpu.py (golden g14 / g14b); here its cost, on rank 0 at N = 1
    if args.full and world == 1 and not args.no_config4:
        try:
            c4 = cases.CFG4
            swin4 = helpers.build_swin(dev, variant=cases.SWIN_B)
            head4 = helpers.build_head(c4, dev, return_aux=False, **cases.CFG4_DECODER)
            tg4 = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in cases.cfg4_targets(c4)[0].items()}

            @torch.no_grad()
            def step4():
                x4 = ops.normalize_pad(frames, mean, std, pad_to=(736, 1280))
                return head4(swin4(x4), targets=[dict(tg4)])
            for _ in range(2):
                step4()
            sync()
            t0 = time.perf_counter()
            for _ in range(5):
                step4()
            sync()
            dt4 = (time.perf_counter() - t0) / 5
            t0 = time.perf_counter()
            step4()
            enq4 = time.perf_counter() - t0
            sync()
            res["config4_swinb_refvos"] = {
                "workload": "BASELINE config 4: Swin-B (12 x 12 windows), T=5 @ 720p (736x1280 padded), 200 queries + 4 referring "
                            "expressions (grounding: lang->vision cross-attention, ProCA, 'sep-blocked' self-attention); 2 warm-up + 5 timed clips",
                "ms_per_clip": dt4 * 1e3, "frames_per_s": c4["T"] / dt4, "queries": c4["Q"] + c4["n_exp"], "host_enqueue_ms": enq4 * 1e3}
            res["config4_swinb_refvos"].update(op_rooflines(ops, step4, sync, c4["T"], 23 * 40 + 46 * 80 + 92 * 160,
                                                            c4["Q"] + c4["n_exp"], 256, 184, 320))
            del swin4, head4
            torch.cuda.empty_cache()
        except Exception as e:  # pragma: no cover
            res["config4_swinb_refvos"] = {"error": repr(e)[:300]}

    if rank != 0:
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return None
    if not args.full:
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return json.dumps(res)

    # ---- parity of the timed path against the reference's own CPU run (tests/golden/g12)
    try:
        import numpy as np
        g = np.load(os.path.join(ROOT, "tests", "golden", "g12_cfg2_full_size.npz"))
        got = out["pred_masks"][0, :, :, ::16, ::16].cpu().numpy()
        res["mask_logit_max_abs_err"] = float(np.abs(got - g["pred_masks_s"]).max())
        res["mask_sign_flips"] = int((((got > 0) != (g["pred_masks_s"] > 0)) & (np.abs(g["pred_masks_s"]) > 1e-3)).sum())
    except Exception as e:  # pragma: no cover
        res["mask_logit_max_abs_err"] = None
        res["parity_note"] = f"golden unavailable: {e}"

    # (a failure in this instrumentation must not cost the headline line: it is reported as `roofline_error` instead)
    try:
        # ---- per-kernel times: a separate instrumented pass AFTER the timed region (rank 0 only)
        def shape_key(t):
            return tuple(t.shape[-2:])

        t_msda = OpTimer(ops, "ms_deform_attn_forward", after=ops.msda_last_tiled_generation)
        t_msdas = OpTimer(ops, "msda_forward_strips", keep_args=6)       # one clip = six encoder layers
        t_msdah = OpTimer(ops, "msda_forward_heads", keep_args=6, after=ops.msda_last_tiled_generation)   # generation 6 (the default)
        t_mdec = OpTimer(ops, "mask_decode", after=ops.mask_decode_last_impl)
        t_mattn = OpTimer(ops, "mask_decode_attn", key=lambda e, f, deferred=False: ("attn",) + shape_key(f), after=ops.mask_decode_last_impl)
        t_res = OpTimer(ops, "bilinear_resample",
                        key=lambda x, size, addend=None: ("fpn" if addend is not None else "maskfeat",) + tuple(int(v) for v in size))
        t_pyr = OpTimer(ops, "bilinear_pyramid3")          # the three mask-feature resamplings of the prediction heads in one pass
        t_win = OpTimer(ops, "window_attention_image",
                        key=lambda qkv, qb, bias, sm, H, W, ws, shift, scale, mma="f32": (int(H), int(W), int(qkv.shape[3]), int(qkv.shape[4])))
        timers = [t_msda, t_msdas, t_msdah, t_mdec, t_mattn, t_res, t_pyr, t_win]
        PROF_STEPS = 5
        for t_ in timers:
            t_.enabled = True
        for _ in range(PROF_STEPS):
            step()
        sync()
        for t_ in timers:
            t_.enabled = False

        # An event pair costs the stream a few microseconds of its own (two marker packets): measured with empty pairs and
        # subtracted from every per-operator figure below, so that a number is the GPU time of the operator's kernels as
        # rocprofv3's kernel trace of the same command reports them (profiles/r03_bench_cfg2_kernel_stats_v5.csv); the raw
        # event-pair figures are reported next to the corrected ones.
        pairs = []
        for _ in range(200):
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            e0.record()
            pairs.append((s0, e0))
        sync()
        ovh = sorted(a_.elapsed_time(b_) for a_, b_ in pairs)[len(pairs) // 2] * 1e-3
        del pairs

        def net(sec_, calls_=1):
            """event-pair seconds of `calls_` operator calls -> seconds without the pairs' own cost"""
            return max(sec_ - calls_ * ovh, 0.5 * sec_)
        ovh_note = f"minus the cost of an empty event pair per operator call ({ovh * 1e6:.1f} us, median of 200)"

        S = 23 * 40 + 46 * 80 + 92 * 160
        alg = 3200.0 * S * T   # bytes per launch (one launch = T frames of one encoder layer)
        t_hm = t_msdah if set(t_msdah.notes.get("all", [])) == {6} else t_msdas     # the head-major operator that ran (generation 6, else 5)
        sec, n = t_hm.seconds()
        fused = bool(n)          # the head-major operator also does msda_prepare's work
        sec_events = sec
        timing = f"HIP events around each launch in a separate pass of {PROF_STEPS} clips after the timed region"
        sec_replay = None
        if fused:
            # the replay of the six launches back to back (operands warm in the memory-side cache) is reported next to it
            sec = net(sec_events)
            timing += "; " + ovh_note
            sec_replay, n_r = t_hm.replay()
            t_hm.args.clear()
        if not n:
            sec, n = t_msda.seconds()
            sec_events = sec
        if n:
            gens = set(t_msda.notes.get("all", []))
            gen = (6 if t_hm is t_msdah else 5) if fused else (max(gens) if gens else 0)
            kname = {6: "msda_fwd_heads<3> (MSDeformAttn core on head-major operands: a lane owns a sample of a full head, one 8-wave "
                        "workgroup per CU with the windows of a 16 x 6 tile resident, the workgroups of an XCD walk adjacent tile columns "
                        "in lockstep)",
                     5: "msda_fwd_strips<3> (MSDeformAttn core on head-major operands: strips with resident row-circular windows at half a "
                        "head per workgroup, two workgroups per CU, a lane owns a sample)",
                     2: "msda_fwd_tiled2<3> (MSDeformAttn forward: LDS-tiled, persistent, producer/consumer waves)"}.get(gen, "msda_fwd_vec4 (generic)")
            res["roofline"] = {"kernel": kname + (" + fused msda_prepare" if fused else ""), "bound": "hbm",
                               "achieved": alg / sec / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": alg / sec / HBM_PEAK,
                               "traffic": None, "avg_launch_us": sec * 1e6, "launches_per_step": n // PROF_STEPS,
                               "algorithmic_bytes_per_launch": alg, "timing": timing,
                               "event_pair_us": sec_events * 1e6,
                               "replay_back_to_back_us": None if sec_replay is None else sec_replay * 1e6}
            if fused:
                # the fused operator also does msda_prepare's work (softmax + reference + offset / normaliser): SURVEY 8d's
                # 3200*S prices the sampling operator alone; un-fused accounting adds the bytes the separate pass would move
                # (the merged projection row in, locations + weights out: 4 * S * T * M * L * P * 3 * 2 bytes)
                prep = 4.0 * S * T * 8 * 3 * 4 * 3 * 2
                res["roofline"]["unfused_accounting"] = {"algorithmic_bytes_per_launch": alg + prep,
                                                         "achieved": (alg + prep) / sec / 1e9, "frac": (alg + prep) / sec / HBM_PEAK}
            # HBM bytes per launch from the PMC passes (rocprofv3 cannot run inside this process): the committed
            # measurement of the same kernel on the same geometry, corrected as the microarch guide prescribes
            for fn in ("r06_msda_traffic.json", "r05_msda_traffic.json", "r04_msda_traffic.json", "r03_msda_traffic.json", "r02_msda_traffic.json", "r01_msda_traffic.json"):
                try:
                    with open(os.path.join(ROOT, "profiles", fn)) as f:
                        tr = json.load(f)
                    if abs(tr["algorithmic_bytes_per_launch"] - alg) < 1 and tr.get("tiled_generation", 2) == gen:
                        res["roofline"]["traffic"] = tr["fetch_bytes_corrected"] + tr["write_bytes"]
                        res["roofline"]["traffic_source"] = f"profiles/{fn} (separate --pmc passes; reads = TCC_EA0_RDREQ_DRAM_32B x 32 B = 2 x FETCH_SIZE, calibrated on known byte counts: profiles/r05_fetch_size_calibration_v1.txt)"
                        break
                except (OSError, KeyError, ValueError):
                    pass

        H, W, C = 184, 320, 256
        sec_md_events, n_md = t_mdec.seconds()
        if n_md:
            sec_md = net(sec_md_events)
            algb = 4.0 * (C * H * W + Q * C + Q * H * W) * T
            flops = 2.0 * Q * C * H * W * T
            impl = set(t_mdec.notes.get("all", []))
            if impl == {2}:
                # fp32 emulated on the bf16 matrix cores (6 bf16 products per fp32 product): HBM-bound, as SURVEY 8d prices it
                res["roofline_mask_decode"] = {"kernel": "skinny_gemm_bf16x6_n32<7,8,Store2Logits> (mask decode: fp32 from an exact 3-way bf16 split, bf16 MFMA)",
                                               "bound": "hbm", "achieved": algb / sec_md / 1e9, "peak": HBM_PEAK / 1e9,
                                               "unit": "GB/s", "frac": algb / sec_md / HBM_PEAK,
                                               "algorithmic_bytes_per_launch": algb, "fp32_equivalent_TFLOPs": flops / sec_md / 1e12,
                                               "bf16_mfma_TFLOPs": 6.0 * flops * (112.0 / Q) / sec_md / 1e12,
                                               "avg_launch_us": sec_md * 1e6, "event_pair_us": sec_md_events * 1e6,
                                               "timing": "HIP events around the launch, " + ovh_note}
            else:
                res["roofline_mask_decode"] = {"kernel": "skinny_gemm_f32<4,StoreLogits> (mask decode, f32 MFMA)",
                                               "bound": "mfma", "achieved": flops / sec_md / 1e12, "peak": F32_MFMA_PEAK / 1e12,
                                               "unit": "TFLOP/s", "frac": flops / sec_md / F32_MFMA_PEAK,
                                               "hbm_GBps": algb / sec_md / 1e9, "avg_launch_us": sec_md * 1e6}
            # the ten prediction-head calls of a clip: un-fused op-boundary bytes over everything we run for them
            n_attn = sum(len(v) for v in t_mattn.events.values())
            n_rs = sum(len(v) for kk, v in t_res.events.items() if kk[0] == "maskfeat") + sum(len(v) for v in t_pyr.events.values())
            fam_events = {"full_res_decode": t_mdec.total_seconds() / PROF_STEPS,
                          "attn_mask": t_mattn.total_seconds() / PROF_STEPS,
                          "mask_feature_resample": (t_res.total_seconds(lambda kk: kk[0] == "maskfeat") + t_pyr.total_seconds()) / PROF_STEPS}
            fam = {"full_res_decode": net(fam_events["full_res_decode"], n_md / PROF_STEPS),
                   "attn_mask": net(fam_events["attn_mask"], n_attn / PROF_STEPS),
                   "mask_feature_resample": net(fam_events["mask_feature_resample"], n_rs / PROF_STEPS)}
            calls = n_md // PROF_STEPS + n_attn // PROF_STEPS
            fam_t = sum(fam.values())
            unfused = 10.0 * algb
            per_level = {}
            for kk in sorted(t_mattn.events):
                s_, n_ = t_mattn.seconds(kk)
                per_level[f"{kk[1]}x{kk[2]}"] = {"avg_launch_us": net(s_) * 1e6, "event_pair_us": s_ * 1e6, "launches_per_step": n_ // PROF_STEPS,
                                                 "impl": sorted(set(t_mattn.notes.get(kk, [])))}
            actual = algb + sum(
                4.0 * T * (C * kk[1] * kk[2] + Q * C) + T * Q * kk[1] * kk[2] for kk in t_mattn.events for _ in
                range(len(t_mattn.events[kk]) // PROF_STEPS)) + sum(
                4.0 * T * C * (H * W + kk[1] * kk[2]) for kk in t_res.events if kk[0] == "maskfeat") + (
                4.0 * T * C * (H * W + sum(kk[1] * kk[2] for kk in t_mattn.events)) if t_pyr.events else 0.0)
            res["roofline_mask_decode_family"] = {
                "what": "10 prediction-head calls per clip (1 full-resolution decode + 9 attention masks at 3 resolutions -- their "
                        "all-masked-row rule is applied inside the cross-attention kernel, no pass of its own -- + the resampling of the mask features to the 3 resolutions: one pass).  `frac` is on the bytes "
                        "these kernels move; `unfused_accounting` is SURVEY.md 8d's (ten full-resolution contractions), which the path "
                        "beats by construction: the attention masks are contracted at 1/8 - 1/32 resolution on pre-resampled features",
                "bound": "hbm", "bytes_per_clip": actual, "seconds_per_clip": fam_t, "achieved": actual / fam_t / 1e9,
                "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": actual / fam_t / HBM_PEAK, "head_calls_per_clip": calls,
                "unfused_bytes_per_clip": unfused,
                "unfused_accounting": {"bytes_per_clip": unfused, "achieved": unfused / fam_t / 1e9, "frac": unfused / fam_t / HBM_PEAK},
                "ms_per_clip": {k: v * 1e3 for k, v in fam.items()}, "attn_mask_per_level": per_level,
                "event_pair_ms_per_clip": {k: v * 1e3 for k, v in fam_events.items()},
                "timing": "HIP events around each operator call (an attention-mask call = the contraction; the rule for fully masked rows is applied by the cross-attention kernel that reads the mask; the last head's: flag memset + contraction + row reset), " + ovh_note,
                "actual_bytes_per_clip_estimate": actual}

            if "roofline" in res:
                # north_star's target object: MSDeformAttn sampling + the prediction-head family of one clip against 8 TB/s,
                # both in SURVEY 8d's accounting (3200 * S * T per MSDA launch, ten full-resolution contractions): >= 0.50 /
                # <= 1.5 ms per clip
                rl = res["roofline"]
                t_ms = rl["avg_launch_us"] * 1e-6 * rl["launches_per_step"]
                b_ms = alg * rl["launches_per_step"]
                res["roofline_msda_plus_mask_decode"] = {
                    "accounting": "SURVEY.md 8d (un-fused op-boundary bytes)",
                    "bound": "hbm", "bytes_per_clip": b_ms + unfused, "ms_per_clip": (t_ms + fam_t) * 1e3,
                    "achieved": (b_ms + unfused) / (t_ms + fam_t) / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                    "frac": (b_ms + unfused) / (t_ms + fam_t) / HBM_PEAK,
                    "parts_ms": {"msda": t_ms * 1e3, "mask_decode_family": fam_t * 1e3}}

        if t_win.events:
            stages = {}
            for kk in sorted(t_win.events, reverse=True):
                s_ev, n_ = t_win.seconds(kk)
                s_ = net(s_ev)
                Hs, Ws, nH, hd = kk
                byts = 4.0 * T * Hs * Ws * nH * hd * 4      # qkv in (3x) + out (1x), fp32
                stages[f"{Hs}x{Ws}x{nH}h"] = {"avg_launch_us": s_ * 1e6, "event_pair_us": s_ev * 1e6, "launches_per_step": n_ // PROF_STEPS,
                                              "algorithmic_bytes_per_launch": byts, "achieved_GBps": byts / s_ / 1e9,
                                              "frac": byts / s_ / HBM_PEAK}
            wa_kernel = {"f16x3": "window_attn_img_f16<4,false,3> (Swin window attention in image order, 7x7 windows: persistent per head, bias table "
                                  "in LDS, two fp16 parts per operand and three products on the fp16 matrix cores: fp32-accurate)",
                         "f32": "window_attn_img7_f32 (Swin window attention in image order, 7x7 windows: persistent per head, bias table in LDS, "
                                "f32 MFMA 16x16x4)"}.get(next((m.mma for m in swin.modules() if hasattr(m, "mma")), "f32"), "window attention")
            res["roofline_window_attn"] = {"kernel": wa_kernel,
                                           "bound": "hbm", "peak": HBM_PEAK / 1e9, "unit": "GB/s", "per_stage": stages,
                                           "ms_per_clip": net(t_win.total_seconds() / PROF_STEPS,
                                                              sum(len(v) for v in t_win.events.values()) / PROF_STEPS) * 1e3,
                                           "event_pair_ms_per_clip": t_win.total_seconds() / PROF_STEPS * 1e3,
                                           "timing": "HIP events around each launch, " + ovh_note}
    except Exception as e:  # pragma: no cover
        import traceback
        res["roofline_error"] = "".join(traceback.format_exception(type(e), e, e.__traceback__))[-1500:]
        for t_ in locals().get("timers", []):
            t_.enabled = False

    if world == 1:
        # informational: a steady-state clip of the same video (second clip, 10 visual-prompt entities in the memory
        # pool -> 110 queries, prompt sampler + ProCA active); the headline `value` stays the BASELINE config
        try:
            case_p = dict(case, H=736, W=1280)
            tv0 = cases.targets_with_entities(case_p, first_frame_idx=1, n_ent=10)[0]
            tvd = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in tv0.items()}
            x_p = torch.nn.functional.pad((frames - mean) / std, (0, 0, 0, 16))
            with torch.no_grad():
                def prompted_clip():
                    torch.manual_seed(0)
                    tg = [dict(tvd)]
                    head.prefetch_prompts(tg, T)          # sampler work that needs the annotations only, ahead of the backbone
                    return head(swin(x_p), targets=tg)
                for _ in range(2):
                    prompted_clip()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    prompted_clip()
                torch.cuda.synchronize()
            dtp = (time.perf_counter() - t0) / 5
            enc_p = head.predictor.visual_prompt_sampler.visual_prompt_encoder
            res["steady_state_with_prompts"] = {"ms_per_clip": dtp * 1e3, "frames_per_s": T / dtp, "entities": 10,
                                                "queries": 110, "sampler": enc_p._rng(dev),
                                                "note": "second clip of a video, visual prompts; the library's default sampler mode"}
            if enc_p._rng(dev) != "reference":
                old_mode = enc_p.sampler_rng
                enc_p.sampler_rng = "reference"
                try:
                    with torch.no_grad():
                        for _ in range(2):
                            prompted_clip()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(5):
                            prompted_clip()
                        torch.cuda.synchronize()
                    res["steady_state_with_prompts"]["reference_sampler_ms_per_clip"] = (time.perf_counter() - t0) / 5 * 1e3
                finally:
                    enc_p.sampler_rng = old_mode
        except Exception as e:  # pragma: no cover
            res["steady_state_with_prompts"] = {"error": str(e)[:200]}

    if world == 1 and not args.no_cpu_baseline:
        # the build's CPU restatement (oracle/cpu_path.py: ATen CPU + plain-C MSDA) on the host cores,
        # 1 warm-up + 3 timed clips, median
        from oracle.cpu_path import cpu_ops
        swin_c = helpers.build_swin("cpu")
        head_c = helpers.build_head(case, "cpu", return_aux=False)
        fr = cases.cfg2_frames()

        def cpu_clip():
            with cpu_ops(), torch.no_grad():
                t1 = time.perf_counter()
                head_c(swin_c(cases.preprocess(fr)), targets=cases.targets_first_clip(case))
                return time.perf_counter() - t1

        # thread count: SURVEY 8d says os.cpu_count(); measured on the GPU box (2 x EPYC 9575F, 256 hardware threads;
        # profiles/r02_bench_cfg2_n1_v1.json) one clip takes 182.7 s with all 256 threads (ATen's CPU kernels oversubscribe on
        # this model's many small ops) and 8.9 s with 32.  So the leg times 32 / 64 / 128 threads (one warm-up + one timed clip
        # each; a count whose warm-up is already 2x slower than the best so far is dropped) and reports the BEST count, with two
        # more timed clips there (median of three); --cpu-threads N pins the count.
        ncpu = os.cpu_count() or 1
        # never more threads than the process may use: its affinity mask, and OMP_NUM_THREADS where the caller set it
        omp = os.environ.get("OMP_NUM_THREADS", "").split(",")[0]
        usable = min(len(os.sched_getaffinity(0)), int(omp) if omp.isdigit() and int(omp) > 0 else ncpu)
        cands = [args.cpu_threads] if args.cpu_threads > 0 else sorted({min(usable, c) for c in (32, 64, 128)})
        sweep, timed = {}, {}
        for c_ in cands:
            torch.set_num_threads(c_)
            os.environ["OMP_NUM_THREADS"] = str(c_)
            sweep[c_] = cpu_clip()                                # warm-up at this count
            if timed and sweep[c_] > 2.0 * min(min(v) for v in timed.values()):
                continue
            timed[c_] = [cpu_clip()]
        cores = min(timed, key=lambda c_: min(timed[c_]))
        torch.set_num_threads(cores)
        os.environ["OMP_NUM_THREADS"] = str(cores)
        runs = sorted(timed[cores] + [cpu_clip() for _ in range(2)])
        res["cpu_baseline"] = {"value": T / runs[1], "unit": "frames/s", "cores": cores, "kind": "port",
                               "cpu": cpu_model_name(), "hardware_threads": ncpu,
                               "sample": "config-2 clips (5 frames) through the CPU oracle path (oracle/cpu_path.py: ATen CPU + "
                                         "plain-C MSDA) at 32 / 64 / 128 threads (1 warm-up + 1 timed each), the best count "
                                         "reported: median of 3 timed clips",
                               "seconds_per_clip": runs,
                               "seconds_per_clip_by_threads": {str(k): min(v) for k, v in timed.items()},
                               "warmup_seconds_by_threads": {str(k): v for k, v in sweep.items()}}
        res["speedup_vs_cpu_baseline"] = res["value"] / res["cpu_baseline"]["value"]   # reported, not a quality measure
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return json.dumps(res)


if __name__ == "__main__":
    main()
