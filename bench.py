#!/usr/bin/env python3
"""Benchmark of the DiffSHEG sampling hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W [--mode batch|chain|ddpm]
  (N > 1: one rank per GPU under torch.distributed.run; started WITHOUT a launcher, it launches the N ranks itself)

Modes (BASELINE.json configs):

  batch  (default, configs[2]; the configuration the headline metric is quoted on)  A "step" is one ``generate_batch``
         (set_condition + ddim25 loop = 25 UniDiffuser evaluations, CFG 1.25) over 950 SHOW clips of n_poses=88 per GPU,
         bf16 storage / bf16 MFMA with fp32 accumulation.  N GPUs = N independent batches: WEAK scaling.
  chain  (configs[3])  A step is one pass over a fixed 9000-frame (5 min @ 30 fps) feature stream through
         ``sample_arbitrary_len_sharded``: overlap_len 10, jump schedule (3,5), the stream cut into --chains independent
         window chains that are sharded over the ranks and gathered on rank 0 (RCCL).  Total work is fixed: STRONG scaling.
  ddpm   (configs[4])  A step is one 1000-step ancestral ``p_sample_loop`` over 2500 SHOW clips split 312/313 per GPU
         (``shard_range``), bf16.  Total work is fixed: STRONG scaling.

Inputs (mel, HuBERT, speaker one-hots) are resident in HBM before the timed region; Gaussian noise comes from the
on-device Philox generator.  Batch rows / chains never couple, so only the timing contract's barrier +
max-reduce (and the chain mode's output gather) use RCCL.

Rank 0 prints ONE JSON line: metric/value (motion frames/s, whole job) and ms_per_step.  A plain run does nothing else: set-up,
--warmup untimed steps, --steps timed steps, the line.

  --full   also measures, beside the headline: the shader clock / socket power of the timed region, the host's own launch cost
           per step (batch mode), and at N=1 in batch mode, outside the timed region: the rooflines of the dominant HBM-bound and
           the largest MFMA-bound kernel instantiation (HIP-event timed on the context stream during one extra instrumented
           single-stream step), the bf16 end-to-end error against the reference golden, the window-chain latencies of config 4
           (first / chained window at 1 chain and at 16 batched chains) and the CPU baselines (the oracle port on the host cores:
           a bounded sample of this workload, and BASELINE config 1 in full).  --no-roofline / --no-chain-latency /
           --no-cpu-baseline drop single legs of it.
  --dump-outputs DIR   after the timed steps, rank 0 writes what the last timed step returned as DIR/samples.npy (float32;
           [clips, frames, channels], or [1, frames, channels] in chain mode).  Above 60 MiB it keeps a fixed, seeded sample of
           whole clips (rows of dim 0; frames of dim 1 when dim 0 is 1), in their original order.  Inputs, weights and noise
           seeds depend only on the arguments, so two builds run with the same arguments can be compared array for array.
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3}     # dense, MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0                                  # HBM3E spec (6.3 TB/s is the measured copy ceiling)
DUMP_BUDGET_BYTES = 60 * 2**20                         # --dump-outputs: larger outputs are written as a seeded sample
DUMP_SAMPLE_SEED = 20240101


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", default="batch", choices=["batch", "chain", "ddpm"])
    ap.add_argument("--batch", type=int, default=None, help="batch mode: clips per GPU (950); ddpm mode: clips in TOTAL (2500)")
    ap.add_argument("--dataset", default="show", choices=["show", "beat"])
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--sampler", default="ddim25", choices=["ddim25", "ddpm1000"], help="batch mode only")
    ap.add_argument("--stream-frames", type=int, default=9000, help="chain mode: length of the feature stream")
    ap.add_argument("--chains", type=int, default=32, help="chain mode: independent chains the stream is cut into (all ranks together)")
    ap.add_argument("--inputs-on-rank0", action="store_true", help="chain mode: only rank 0 holds the feature stream; it is broadcast (RCCL) first")
    ap.add_argument("--full", action="store_true", help="also run the measurements beside the headline (telemetry, launch cost, "
                                                             "roofline, chain latencies, CPU baselines); off by default")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's output to DIR/samples.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline step")
    ap.add_argument("--no-chain-latency", action="store_true", help="with --full: skip the window-chain latencies")
    ap.add_argument("--cpu-batch", type=int, default=8, help="clips in the CPU-baseline sample of this workload")
    ap.add_argument("--cpu-config1-steps", type=int, default=1000, help="steps of BASELINE configs[0]'s 1000-step loop timed on the host (1000 = in full)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    return args


def dump_outputs(out: torch.Tensor, out_dir: str) -> dict:
    """--dump-outputs: the last timed step's samples as out_dir/samples.npy, float32.  Above DUMP_BUDGET_BYTES only a fixed,
    seeded subset of whole clips (dim 0, or dim 1 when dim 0 is 1) is written, sorted so it keeps the original order."""
    import numpy as np
    x = out.detach().float()
    axis = 0 if x.shape[0] > 1 else 1
    n = x.shape[axis]
    per_row = x.numel() // n * 4
    keep = min(n, DUMP_BUDGET_BYTES // per_row)
    rows = None
    if keep < n:
        rows = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, size=keep, replace=False))
        x = x.index_select(axis, torch.from_numpy(rows).to(x.device))
    arr = np.ascontiguousarray(x.cpu().numpy(), dtype=np.float32)
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "samples.npy"), arr)
    return {"dir": out_dir, "samples": {"shape": list(arr.shape), "dtype": "float32", "full_shape": list(out.shape),
                                        "sampled_axis": axis if rows is not None else None,
                                        "sample": None if rows is None else f"{keep} of {n}, numpy default_rng({DUMP_SAMPLE_SEED}) choice, sorted"}}


def cpu_baseline(cfg, sd, n_clips: int, full_batch: int):
    """Oracle port (oracle/, plain PyTorch fp32) on the host cores: one ddim25 pass over a SAMPLE of n_clips clips."""
    from diffsheg_amd.synthetic import make_inputs
    from oracle import denoiser_ref, sampler_ref
    threads = torch.get_num_threads()
    inp = make_inputs(cfg, n_clips, seed=3)
    B, T = n_clips, cfg.n_poses

    def eps_fn(xc, t_orig, c1, c2):
        with torch.no_grad():
            return denoiser_ref.unidiffuser(sd, cfg, xc, torch.full((B,), t_orig), c1, c2, inp["audio_emb"],
                                            inp["person_id"], inp["pretrain_aud_feat"])
    t0 = time.perf_counter()
    sampler_ref.ddim_sample_loop(eps_fn, (B, T, cfg.net_dim_pose), {}, sampler_ref.NoiseSource(seed=1))
    dt = time.perf_counter() - t0
    return {"value": B * T / dt, "unit": "frames/s", "cores": threads, "kind": "port",
            "sample": f"REDUCED-BATCH SAMPLE of the bench workload: oracle port (plain PyTorch fp32 on the host, {threads} threads of "
                      f"{os.cpu_count()} logical cores), one ddim25 pass (25 evals) of {cfg.dataset} n_poses={T} CFG {cfg.cond_scale} at "
                      f"batch {B} instead of {full_batch}: {dt:.1f} s; frames/s is per-clip throughput at this batch, i.e. a linear "
                      f"extrapolation to batch {full_batch} (the CPU is already compute-bound at batch {B})"}


def cpu_baseline_config1(n_steps: int):
    """BASELINE configs[0] (BEAT n_poses=34, batch 1, 1000-step ancestral loop), oracle port on the host.  The default bench
    times the loop in full (~0.5 min on 16 threads); ``--cpu-config1-steps n`` times a prefix of n steps
    (every step costs the same: one B=1 denoiser evaluation + the update) and scales it.  Batch-1 evaluations
    do not scale past a few cores (oversubscribing 128 threads made the full loop take 8.5 min on the MI355X host), so the
    thread count is capped at 16."""
    from diffsheg_amd.config import get_config
    from diffsheg_amd.synthetic import make_inputs
    from diffsheg_amd.weights import make_synthetic_state_dict
    from oracle import denoiser_ref, sampler_ref
    cfg = get_config("beat")
    sd = make_synthetic_state_dict(cfg, 1234)
    inp = make_inputs(cfg, 1, seed=3)
    all_threads = torch.get_num_threads()
    threads = min(16, all_threads)
    torch.set_num_threads(threads)
    try:
        tb = sampler_ref.diffusion_tables(sampler_ref.linear_betas(1000))
        src = sampler_ref.NoiseSource(seed=1)
        x = src.randn((1, cfg.n_poses, cfg.net_dim_pose))
        t0 = time.perf_counter()
        for t in range(999, 999 - n_steps, -1):
            c1, c2 = sampler_ref._f32(tb["sqrt_recip_alphas_cumprod"], t), sampler_ref._f32(tb["sqrt_recipm1_alphas_cumprod"], t)
            with torch.no_grad():
                eps = denoiser_ref.unidiffuser(sd, cfg, x, torch.full((1,), t), c1, c2, inp["audio_emb"], inp["person_id"], inp["pretrain_aud_feat"])
            x, _ = sampler_ref.ddpm_step(tb, t, x, eps, src)
        dt = time.perf_counter() - t0
    finally:
        torch.set_num_threads(all_threads)
    full = dt * 1000.0 / n_steps
    how = "the loop in full" if n_steps == 1000 else f"the first {n_steps} of the 1000 steps ({dt:.1f} s), scaled x{1000 / n_steps:g}"
    return {"value": cfg.n_poses / full, "unit": "frames/s", "cores": threads, "kind": "port",
            "sample": f"BASELINE configs[0]: BEAT n_poses=34, batch 1, 1000-step p_sample_loop, oracle port on {threads} threads of "
                      f"{os.cpu_count()} logical cores: {how} = {full:.1f} s per 34-frame clip"}


def gpu_config1(dev: str):
    """BASELINE configs[0] on the GPU, next to its CPU line: BEAT n_poses=34, batch 1, the 1000-step ancestral loop on the fp32 path
    (the <= 1e-3 parity configuration; tests/test_gpu_sampler.py pins exactly this loop against ddpm1000_beat.npz).  One warm-up
    pass, then the median of three; a latency figure (one clip), not a throughput one."""
    from diffsheg_amd.config import get_config
    from diffsheg_amd.model import UniDiffuser
    from diffsheg_amd.synthetic import make_inputs
    from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace
    from diffsheg_amd.weights import make_synthetic_state_dict
    cfg = get_config("beat")
    model = UniDiffuser(cfg, make_synthetic_state_dict(cfg, 1234), device=dev, precision="fp32")
    tr = DDPMTrainer(sampler_namespace(cfg, ddim=False), model)
    inp = make_inputs(cfg, 1, seed=3)
    audio, pid = inp["audio_emb"].to(dev), inp["person_id"].to(dev)
    add = {"pretrain_aud_feat": inp["pretrain_aud_feat"].to(dev)}
    times = []
    for i in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.generate_batch(audio, pid, cfg.net_dim_pose, add, {}, seed=11 + i)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt = sorted(times[1:])[1]
    del tr, model
    return {"value": cfg.n_poses / dt, "unit": "frames/s", "latency_s": dt, "dtype": "fp32",
            "sample": f"BASELINE configs[0] on this GPU: BEAT n_poses=34, batch 1, 1000-step p_sample_loop, fp32 path, median of 3 after a "
                      f"warm-up: {dt * 1e3:.0f} ms per 34-frame clip ({dt:.3f} ms per step) — the same workload as cpu_baseline_config1"}


def golden_rel_err(model, cfg, tr):
    """Replay tests/golden/ddim25_plain_show.npz (generated from the imported reference by tests/golden/make_golden.py: seeds +
    expected final sample) on the benchmark's model: max |x - ref| / max |ref| and rms error / rms of the whole ddim25 loop."""
    import numpy as np
    from diffsheg_amd.synthetic import SeededNoise, make_inputs
    path = os.path.join(ROOT, "tests", "golden", "ddim25_plain_show.npz")
    if not os.path.exists(path):
        return None
    f = np.load(path)
    B = int(f["batch"])
    inp = make_inputs(cfg, B, seed=int(f["input_seed"]))
    kw = {"audio_emb": inp["audio_emb"], "length": None, "person_id": inp["person_id"],
          "add_cond": {"pretrain_aud_feat": inp["pretrain_aud_feat"]}, "y": {}, "pe_type": "pe_sinu"}
    model._cond_key = None
    x = tr.diffusion_ddim_val.ddim_sample_loop(model, (B, cfg.n_poses, cfg.net_dim_pose), clip_denoised=False, model_kwargs=kw,
                                               noise_source=SeededNoise(int(f["noise_seed"])))
    ref = torch.from_numpy(f["final"])
    d = x.detach().float().cpu() - ref
    model._cond_key = None
    return {"max_err_over_range": float(d.abs().max() / ref.abs().max()), "rms_err_over_rms": float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()),
            "fixture": "tests/golden/ddim25_plain_show.npz (reference golden, B = 2, recorded noise)"}


def self_launch(n: int) -> int:
    """``python bench.py --gpus N`` without a launcher: re-run this command line as N ranks of one node under
    torch.distributed.run (what the reference does with mp.spawn, runner.py:80-122) and return its exit code."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def dry_run(args, rank: int, world: int):
    """DSH_BENCH_DRYRUN=1 (tests of the launch plumbing on GPU-less hosts): rendezvous over gloo, the timing contract's
    barrier + max-reduce, ONE JSON line from rank 0 — and no sampling at all; the line says so and carries no throughput."""
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo")
        dist.barrier()
    t = torch.tensor([1.0 + rank], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(json.dumps({"metric": "DRY RUN (launch plumbing only, nothing was sampled)", "value": None, "n_gpus": world, "mode": args.mode,
                          "steps": args.steps, "warmup": args.warmup, "dry_run": True, "max_over_ranks": float(t)}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:                       # never print a line whose n_gpus differs from what was asked for
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if os.environ.get("DSH_BENCH_DRYRUN") == "1":
        return dry_run(args, rank, world)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    # DSH_BENCH_OVERSUBSCRIBE=1 (single-GPU test boxes): ranks share the visible devices round-robin; RCCL refuses two ranks on one
    # device, so such a run must also set DSH_BENCH_BACKEND=gloo (barrier / max-reduce / gather through the host)
    ndev = torch.cuda.device_count()
    if local_rank >= ndev:
        if os.environ.get("DSH_BENCH_OVERSUBSCRIBE") != "1":
            raise SystemExit(f"rank {rank}: LOCAL_RANK={local_rank} but only {ndev} GPU(s) are visible")
        local_rank %= ndev
    torch.cuda.set_device(local_rank)
    # one launch thread per GPU: keep it on the cores of the socket the GPU hangs off (8 ranks x ~12 k launches per step share one host)
    from diffsheg_amd.hostenv import GpuTelemetry, pin_to_local_numa
    # (multi-rank jobs only: a single rank keeps the whole host — its CPU-baseline legs below use every core, and torch's intra-op pool
    #  was sized for them; pinned to one NUMA node the 128-thread oracle run oversubscribed 4x and the default bench no longer finished
    #  in its 400 s, profiles/r05_j_bench.err)
    affinity0 = os.sched_getaffinity(0) if hasattr(os, "sched_getaffinity") else None
    if world > 1:
        pin = pin_to_local_numa(local_rank, min(ndev, int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))),
                                pci_ids=[GpuTelemetry.pci_bus_id_of(i) for i in range(ndev)])
    else:
        pin = {"pinned": False, "why": "single rank: the launch thread and the CPU-baseline legs keep the whole host"}
    dist = None
    # a process group whenever a launcher started us — also for ONE rank (python -m torch.distributed.run --nproc-per-node 1 bench.py
    # --gpus 1): that is how the RCCL path (init with device_id, barrier, max-reduce, device-side gather) runs on a single-GPU box
    if world > 1 or "RANK" in os.environ:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("DSH_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
        else:
            dist.init_process_group(backend)

    from diffsheg_amd import _lib
    from diffsheg_amd.buildid import kernel_build_id
    from diffsheg_amd.config import get_config
    from diffsheg_amd.model import UniDiffuser
    from diffsheg_amd.synthetic import make_inputs
    from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace, shard_range
    from diffsheg_amd.weights import make_synthetic_state_dict

    cfg = get_config(args.dataset)
    sd = make_synthetic_state_dict(cfg, 1234)
    if os.environ.get("DSH_BENCH_ZERO_DATA") == "1":
        # power probe, never a result: all-zero weights make every MFMA / LDS / HBM operand zero — same instruction stream, far less
        # switching energy.  If the step gets much faster, the chip is clocking to its power budget (MI355X_MICROARCH.md, DVFS).
        sd = {k: torch.zeros_like(v) for k, v in sd.items()}
    dev = f"cuda:{local_rank}"
    model = UniDiffuser(cfg, sd, device=dev, precision=args.precision)
    mode = args.mode
    sampler = "ddpm1000" if mode == "ddpm" else ("ddim25" if mode == "chain" else args.sampler)
    ddim = sampler == "ddim25"
    tr = DDPMTrainer(sampler_namespace(cfg, ddim=ddim), model)
    T, Cc = cfg.n_poses, cfg.net_dim_pose

    def clips(B, seed):
        """B distinct synthetic clips resident on the device."""
        small = make_inputs(cfg, min(B, 64), seed=seed)
        rep = (B + small["audio_emb"].shape[0] - 1) // small["audio_emb"].shape[0]
        audio = small["audio_emb"].repeat(rep, 1, 1)[:B].to(dev).contiguous()
        hubert = small["pretrain_aud_feat"].repeat(rep, 1, 1)[:B].to(dev).contiguous()
        # decorrelate the repeated rows so no two clips are identical
        audio += 0.01 * torch.randn(audio.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed + 4))
        pid = torch.zeros(B, cfg.style_dim, device=dev)
        pid[torch.arange(B), torch.arange(B) % cfg.style_dim] = 1.0
        return audio, hubert, pid

    if mode == "batch":
        B = args.batch or 950
        audio, hubert, pid = clips(B, 3 + rank)                 # distinct clips per rank
        frames_per_step = world * B * T
        scaling = "weak"
    elif mode == "ddpm":
        Btot = args.batch or 2500
        mine = shard_range(Btot, rank, world)
        B = len(mine)
        audio, hubert, pid = clips(B, 3 + rank)
        frames_per_step = Btot * T
        scaling = "strong"
    else:
        N = args.stream_frames
        inp = make_inputs(cfg, 1, frames=N, seed=3)             # the SAME stream on every rank (each rank loads it, like the reference)
        audio, hubert = inp["audio_emb"].to(dev), inp["pretrain_aud_feat"].to(dev)
        pid = inp["person_id"].to(dev)
        B = 0
        frames_per_step = N
        scaling = "strong"
    add_cond = {"pretrain_aud_feat": hubert}

    def step(i):
        model._cond_key = None          # every step is a fresh batch: hubert_encoder / pid_embed are re-run
        if mode == "chain":
            if args.inputs_on_rank0:
                return tr.sample_arbitrary_len_sharded(audio if rank == 0 else None, pid, add_cond if rank == 0 else None, args.chains,
                                                       seed=2024 + 7919 * i, inputs_on_rank0_only=True)
            return tr.sample_arbitrary_len_sharded(audio, pid, add_cond, args.chains, seed=2024 + 7919 * i)
        return tr.generate_batch(audio, pid, Cc, add_cond, {}, seed=2024 + 1000 * rank + i)

    def sync_barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        out = step(-1 - i)
    sync_barrier()
    lat, enq = [], []
    tele = None
    if args.full:
        tele = GpuTelemetry(local_rank, pci_bus_id=GpuTelemetry.pci_bus_id_of(local_rank))
        tele.start()                              # shader clock / socket power of this rank's GPU, sampled over the timed region only
    t0 = time.perf_counter()
    for i in range(args.steps):
        s0 = time.perf_counter()
        out = step(i)
        enq.append(time.perf_counter() - s0)      # host time to ENQUEUE the step (the sampler calls are asynchronous on the context stream)
        if mode != "chain" or world == 1:
            # per-step latency sample of THIS rank: batch / ddpm steps have no cross-rank dependence, so the extra device sync per
            # step changes nothing at N > 1 either (chain mode ends every step with a gather: its step time IS the wall time)
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - s0)
    sync_barrier()
    dt = time.perf_counter() - t0
    if tele is not None:
        tele.stop()
    if out is not None:
        assert torch.isfinite(out).all(), "non-finite samples"
        if mode == "chain":
            assert tuple(out.shape) == (1, args.stream_frames, Cc)
    dumped = dump_outputs(out, args.dump_outputs) if (args.dump_outputs and rank == 0 and out is not None) else None
    if dist is not None:
        tmax = torch.tensor([dt], device=dev if dist.get_backend() == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    frames = frames_per_step * args.steps
    evals_per_step = 25 if ddim else cfg.diffusion_steps
    cfg_txt = f"CFG cond_scale={cfg.cond_scale}" if cfg.cfg_active else "no CFG"
    if mode == "batch":
        which = {("show", "bf16", "ddim25", 950): "BASELINE configs[2]", ("beat", "fp32", "ddim25", 256): "BASELINE configs[1]"}.get(
            (cfg.dataset, args.precision, sampler, B), "not a BASELINE config")
        workload = f"{cfg.dataset.upper()} n_poses={T} {sampler} {cfg_txt} batch={B}/GPU {args.precision} ({which})"
        par = f"{world} independent batch shard(s) of {B} clips, no data-path collective"
    elif mode == "ddpm":
        workload = (f"{cfg.dataset.upper()} n_poses={T} ddpm1000 (p_sample_loop, 1000 evals) {cfg_txt} batch={frames_per_step // T} in total "
                    f"{args.precision} (BASELINE configs[4])")
        par = f"batch rows sharded {'/'.join(str(len(shard_range(frames_per_step // T, r, world))) for r in range(world))} over {world} rank(s), no data-path collective"
    else:
        workload = (f"{cfg.dataset.upper()} test_arbitrary_len on a {args.stream_frames}-frame synthetic stream, overlap_len={cfg.overlap_len}, "
                    f"jump ({cfg.jump_length},{cfg.jump_n_sample}), {args.chains} independent window chains {args.precision} (BASELINE configs[3])")
        par = f"{args.chains} chains sharded over {world} rank(s), equal-length chains batched per rank, outputs gathered to rank 0 (RCCL)"
    result = {
        "metric": "motion frames/sec (ddim25, n_poses=88)" if (ddim and args.dataset == "show") else
                  f"motion frames/sec ({sampler}, n_poses={T})",
        "value": frames / dt, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
        "dtype": args.precision, "data": ("POWER PROBE: all-zero weights — NOT a result" if os.environ.get("DSH_BENCH_ZERO_DATA") == "1" else
                                          "synthetic (seeded N(0,1) mel/HuBERT, one-hot speakers, random-init weights, Philox noise)"),
        "config": {"workload": workload, "mode": mode, "frames_per_step": frames_per_step, "frames_per_clip": T, "channels": Cc,
                   "denoiser_evals_per_window": evals_per_step if mode != "chain" else "25 (first window of a chain) / 63 + 48 undo steps (chained window)",
                   "parallelism": par,
                   "max_streams_per_gpu": 1 if os.environ.get("DSH_DUAL") == "0" else int(os.environ.get("DSH_DUAL") or 3),
                   "stream_note": "batches of >= 64500 token rows (the 950-clip batch of configs[2]: 83600) are sampled as three independent "
                                  "sub-batches, each running the whole loop on its own HIP stream (shared weights; one fork before the loop, "
                                  "one join after it); below that a sampling loop runs the batch as ONE batch with the two encoders' chains on "
                                  "two streams, the gesture encoder one step behind the expression encoder (the expression chain never waits "
                                  "for a gesture evaluation: round 6, DESIGN.md section 4.8); results are bit-identical to one stream either way"},
    }
    result["expected_scaling"] = {
        "batch": "weak scaling, N independent 950-clip batches and no data-path collective: linear in N by construction",
        "ddpm": "strong scaling over batch rows: linear down to ~300 clips per GPU (a launch still covers > 50k token rows)",
        "chain": ("strong scaling over INDEPENDENT chains of one stream (windows of one chain are sequential): a batch of 16 chains costs only "
                  "~1.7x one chain per window (launch-bound regime, the two encoder chains on two streams), so 1 -> 8 GPUs at 32 chains buys "
                  "~1.5 - 2x; >= 6x needs hundreds of chains (many streams), where every GPU still holds a batch large enough to leave that regime"),
    }[mode]
    result["host_enqueue_ms_per_step"] = 1e3 * statistics.median(enq)
    result["host_enqueue_note"] = ("wall time for this rank's host thread to return from one step() call, before any device sync (median); "
                                   "it INCLUDES the time hipLaunchKernel blocks while the device queues are full (rocprofv3 --hip-trace of this "
                                   "command: most launches return in 2 - 8 us, a few block for tens of ms) — host_launch_cost_ms_per_step (--full) is "
                                   "the host's own cost")
    if args.full and mode == "batch" and B > 0:
        # the host's own launch cost, without back-pressure: single evaluations enqueued on an IDLE device (a few hundred launches each, far
        # below the queue depth), timed until the call returns; x 25 (or 1000) evaluations per step
        tt_ = torch.full((B,), 500, dtype=torch.long, device=dev)
        xx_ = torch.zeros(B, T, Cc, device=dev)
        one_ = [torch.ones(B, device=dev), torch.ones(B, device=dev)]
        model._cond_key = None
        model(xx_, tt_, sqrt_alphas=one_, audio_emb=audio, length=None, person_id=pid, add_cond=add_cond, pe_type="pe_sinu", y={})
        torch.cuda.synchronize()
        es = []
        for _ in range(5):
            s0 = time.perf_counter()
            model(xx_, tt_, sqrt_alphas=one_, audio_emb=audio, length=None, person_id=pid, add_cond=add_cond, pe_type="pe_sinu", y={})
            es.append(time.perf_counter() - s0)
            torch.cuda.synchronize()
        evals = 25 if ddim else cfg.diffusion_steps
        result["host_launch_cost_ms_per_step"] = 1e3 * statistics.median(es) * evals
        result["host_launch_cost_note"] = (f"{evals} x the median wall time to ENQUEUE one UniDiffuser evaluation on an idle device (no queue "
                                           "back-pressure): what the launch thread itself costs per step")
        model._cond_key = None
    result["host_affinity"] = pin
    if tele is not None:
        result["telemetry"] = tele.summary()
    if dumped is not None:
        result["dump_outputs"] = dumped
    if lat:
        result["p50_step_latency_ms"] = 1e3 * statistics.median(lat)
        result["step_latency_note"] = f"wall time of one step of this mode on rank 0, median over {len(lat)} steps"
    if dist is not None:
        result["collective_backend"] = dist.get_backend()

    single = args.full and rank == 0 and world == 1 and mode == "batch"
    lib = _lib.lib()
    if single and not args.no_roofline:
        _lib.check(lib.dsh_profile_enable(model._h, 1))
        step(10_000)
        ms = (C.c_double * 16)(); n = (C.c_int64 * 16)(); fl = (C.c_double * 16)(); by = (C.c_double * 16)()
        _lib.check(lib.dsh_profile_read(model._h, ms, n, fl, by))
        _lib.check(lib.dsh_profile_enable(model._h, 0))
        mfma_peak = MFMA_PEAK_TFLOPS[args.precision]
        ridge = (mfma_peak * 1e12) / (HBM_PEAK_GBS * 1e9)           # flop/byte where the two roofs meet
        names, role = {}, {}
        for c in range(16):
            kn, rl = C.c_char_p(), C.c_char_p()
            _lib.check(lib.dsh_profile_class_info(model._h, c, C.byref(kn), C.byref(rl)))
            if kn.value and c not in (1, 2, 3):                       # GEMM-type classes only (attention / row / sampler kernels: separate keys)
                names[c], role[c] = kn.value.decode(), rl.value.decode()
        per = {}
        for c in names:
            if n[c] == 0:
                continue
            sec = ms[c] * 1e-3
            per[names[c]] = {"role": role[c], "ms_per_step": ms[c], "launches": int(n[c]), "avg_launch_us": 1e3 * ms[c] / int(n[c]),
                             "tflops": fl[c] / sec / 1e12, "algorithmic_gb_per_s": (by[c] / sec / 1e9) if by[c] > 0 else None,
                             "flop_per_byte": (fl[c] / by[c]) if by[c] > 0 else None}
        live = [c for c in names if n[c] > 0]

        def block(c, bound):
            sec = ms[c] * 1e-3
            if bound == "hbm":
                ach, peak, unit = by[c] / sec / 1e9, HBM_PEAK_GBS, "GB/s"
            else:
                ach, peak, unit = fl[c] / sec / 1e12, mfma_peak, "TFLOP/s"
            return {"bound": bound, "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak, "traffic": None,
                    "kernel": names[c], "role": role[c], "launches": int(n[c]), "avg_launch_us": 1e3 * ms[c] / int(n[c]),
                    "algorithmic_bytes_per_launch": by[c] / int(n[c]) if by[c] > 0 else None,
                    "flops_per_launch": fl[c] / int(n[c]), "flop_per_byte": (fl[c] / by[c]) if by[c] > 0 else None,
                    "share_of_step": ms[c] / sum(ms[k] for k in range(16))}
        dom = max(live, key=lambda c: ms[c])                          # dominant kernel instantiation by time
        dom_hbm = by[dom] > 0 and fl[dom] / by[dom] < ridge
        result["roofline"] = block(dom, "hbm" if dom_hbm else "mfma")
        result["roofline"]["kernels"] = per
        result["roofline"]["attention_ms_per_step"] = ms[1]
        result["roofline"]["note"] = (
            "dominant kernel instantiation of one instrumented step (full-batch launches on ONE stream, i.e. the kernel in isolation; the "
            "timed steps overlap the launch sequences of three sub-batches), HIP-event timed on the context stream; algorithmic bytes = input rows + "
            "weight + residual + outputs, each moved once; flops = GEMM flops actually issued (skipped CFG-null feat_proj / per-step hubert "
            "conv are not counted); rocprofv3 summaries of the same command: profiles/r05_*_kernel_stats.txt")
        mf = [c for c in live if c != 0 and (by[c] == 0 or fl[c] / by[c] >= ridge)]
        if mf:                                                        # the largest MFMA-bound instantiation, priced against the matrix peak
            result["roofline_mfma"] = block(max(mf, key=lambda c: ms[c]), "mfma")
        # HBM traffic (PMC) cannot be collected inside this run (rocprofv3 --pmc passes are separate processes): the committed
        # per-launch figure is attached only if it was collected on THIS build of the kernels, on this workload.
        bid = kernel_build_id()
        result["kernel_build_id"] = bid
        for blk in ("roofline", "roofline_mfma"):
            if blk not in result:
                continue
            for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_step*.json")), reverse=True):
                try:
                    pj = json.load(open(path))
                except Exception:                                     # noqa: BLE001
                    continue
                # (the profiler's class label may omit trailing template arguments: "tl3_ffn_kernel<false>" is the instantiation
                #  rocprofv3 names "tl3_ffn_kernel<false, true>")
                kmap, label = pj.get("kernels", {}), result[blk]["kernel"]
                pk = kmap.get(label) or next((v for k, v in kmap.items() if k.startswith(label.rstrip(">"))), None)
                if pj.get("kernel_build_id") == bid and pk and "hbm_traffic_bytes" in pk and \
                        (args.dataset, B, args.precision) == ("show", 950, "bf16"):
                    result[blk]["traffic"] = pk["hbm_traffic_bytes"]
                    result[blk]["traffic_source"] = (f"{os.path.relpath(path, ROOT)} (rocprofv3 --pmc FETCH_SIZE x2 gfx950 correction + "
                                                     f"WRITE_SIZE, per launch, same kernel build {bid})")
                    break
        # accuracy of this precision next to its speed: the committed end-to-end figures of the SAME code path against the
        # reference goldens (tests/test_gpu_sampler.py, profiles/r03_*_pytest_gpu*.log).  Only the fp32 path is inside
        # north_star's 1e-3; the bf16 headline is gated at 1.2e-2 of the output range.
        result["parity_note"] = ("fp32 path: ddim25 loops / chains within 1e-3 of the reference's output range (tests: 4e-7 .. 8e-7); "
                                 "bf16 path (this run when dtype = bf16): ddim25 end to end against the reference golden is MEASURED in this "
                                 "run (e2e_rel_err_vs_reference_golden; gate of the test suite 1.2e-2 of range) — a few 1e-3, NOT inside "
                                 "the 1e-3 bar, which SURVEY section 8 applies to fp32")
        # measured in THIS run: the committed reference golden of the plain ddim25 loop (tests/golden/ddim25_plain_show.npz: SHOW,
        # B = 2, recorded noise stack; tests/test_gpu_sampler.py replays the same fixture) sampled by this model object
        result["e2e_rel_err_vs_reference_golden"] = golden_rel_err(model, cfg, tr) if (cfg.dataset == "show" and ddim) else None
        result["bf16_e2e_rel_err"] = (result["e2e_rel_err_vs_reference_golden"] or {}).get("max_err_over_range") if args.precision == "bf16" else None
        tot_fl = sum(fl[c] for c in range(16))
        result["issued_tflop_per_step"] = tot_fl / 1e12
        result["end_to_end_mfma_frac"] = tot_fl / 1e12 / (result["ms_per_step"] * 1e-3) / mfma_peak
        # the same two fractions priced at the shader clock the timed region actually ran at (the peak scales with the clock: 2.5 PF is
        # 2.4 GHz) — BESIDE the nominal ones, never instead of them
        clk = result["telemetry"].get("clock_mhz_mean")
        if clk:
            result["clock_mhz_mean"], result["power_w_mean"] = clk, result["telemetry"].get("power_w_mean")
            result["end_to_end_mfma_frac_at_measured_clock"] = result["end_to_end_mfma_frac"] * 2400.0 / clk
            for blk in ("roofline", "roofline_mfma"):
                if blk in result and result[blk]["bound"] == "mfma":
                    result[blk]["frac_at_measured_clock"] = result[blk]["frac"] * 2400.0 / clk
                    result[blk]["frac_at_measured_clock_note"] = ("frac x 2400 MHz / mean shader clock of the timed region (telemetry); the instrumented "
                                                                  "single-stream step of this block is not sampled separately")

    if single and not args.no_chain_latency and ddim:
        # BASELINE's "p50 clip latency": wall time of one window of the arbitrary-length chain (config 4) — the first window
        # of a chain (un-masked, 25 evals) and a chained one (out-painting: 63 evals + 48 undo steps) — at 1 chain (the
        # reference's real-time use case; B = 1 -> B' = 2 under CFG) and at 16 chains batched on this GPU.
        def med(fn, n_rep=5):
            ts = []
            for i in range(n_rep + 1):
                torch.cuda.synchronize(); s0 = time.perf_counter(); fn(i); torch.cuda.synchronize()
                ts.append(time.perf_counter() - s0)
            return 1e3 * statistics.median(ts[1:])
        L = cfg.overlap_len
        chain = {}
        for G in (1, 16):
            a1, h1, p1 = audio[:G].contiguous(), {"pretrain_aud_feat": hubert[:G].contiguous()}, pid[:G].contiguous()
            y = {"gt": torch.randn(G, T, Cc, device=dev), "outpainting_mask": torch.zeros(G, T, Cc, dtype=torch.bool, device=dev)}
            y["outpainting_mask"][:, :L] = True

            def first(i):
                model._cond_key = None
                tr.generate_batch(a1, p1, Cc, h1, {}, seed=77 + i)

            def chained(i):
                model._cond_key = None
                tr.generate_batch(a1, p1, Cc, h1, y, seed=177 + i)
            f_ms, c_ms = med(first), med(chained)
            chain[f"chains_{G}"] = {"p50_first_window_ms": f_ms, "p50_chained_window_ms": c_ms,
                                    "ms_per_eval_first": f_ms / 25, "ms_per_eval_chained": c_ms / 63,
                                    "frames_per_s_steady_state": G * (T - L) / (c_ms * 1e-3)}
        chain["note"] = (f"one {T}-frame window per chain; first = 25 evals, chained = 63 evals + 48 undo steps (jump (3,5)); steady-state "
                         f"frames/s = {T - L} new frames per chained window per chain; median of 5 after 1 warm-up")
        result["chain_window_latency"] = chain
        result["p50_single_clip_latency_ms"] = chain["chains_1"]["p50_first_window_ms"]
        result["p50_chained_window_latency_ms"] = chain["chains_1"]["p50_chained_window_ms"]

    if single and not args.no_cpu_baseline:
        if affinity0 is not None:
            os.sched_setaffinity(0, affinity0)              # the CPU legs run on every core this process was given
        result["cpu_baseline"] = cpu_baseline(cfg, sd, args.cpu_batch, B)
        result["cpu_baseline_config1"] = cpu_baseline_config1(max(1, min(1000, args.cpu_config1_steps)))
        result["config1_gpu"] = gpu_config1(dev)

    if rank == 0:
        print(json.dumps(result), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
