"""Step time of BCVAE training: the HIP trainer (said_amd.training.BCVAETrainer, graph replay) against the restated reference step
(tests/vae_train_ref.py) in fp32 as torch eager on the same GPU and on the host CPU.

Each configuration runs `--warmup` steps, then `--steps` timed steps; the HIP trainer and torch on the GPU are timed per step with a device
synchronisation around each one (the per-step time includes the host work of the step), the CPU per step with perf_counter.  Prints one JSON
line with the medians (ms) and the spread (min, max).

Usage:  python scripts/bench_vae_train.py [--batches 8 64] [--steps 50] [--warmup 10] [--cpu-threads 16] [--no-cpu]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from said_amd.training import BCVAETrainer, VAEWindowDataset, bcvae_init_state_dict  # noqa: E402
from vae_train_ref import RefTrainer, windows_of  # noqa: E402


def summary(ts):
    ts = [t * 1e3 for t in ts]
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-steps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(args.cpu_threads)
    rng = np.random.default_rng(0)
    seqs = [rng.random((int(n), 32)).astype(np.float32) for n in rng.integers(61, 400, 64)]
    perm = np.arange(32)
    torch.manual_seed(0)
    init = bcvae_init_state_dict()
    total = args.warmup + args.steps
    res = {"name": "bench_vae_train", "device": torch.cuda.get_device_name(0)}
    for B in args.batches:
        items = np.stack([np.stack([rng.integers(0, 64, B), rng.integers(-60, 60, B), rng.integers(0, 2, B), np.zeros(B, int)], 1)
                          for _ in range(total)]).astype(np.int32)
        eps = rng.standard_normal((total, B, 64)).astype(np.float32)
        tr = BCVAETrainer("cuda:0", max_batch=B, num_training_steps=10 * total, state_dict=init)
        tr.set_train_data(VAEWindowDataset(sequences=seqs))
        ts = []
        for k in range(total):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr._step(items[k], eps[k], 1.0, 1.0)
            tr.eng.read_losses(False, reset=False)   # synchronises the trainer's stream
            if k >= args.warmup:
                ts.append(time.perf_counter() - t0)
        # back to back: `steps` steps enqueued, one synchronisation at the end (what train_epoch does)
        tr.eng.read_losses(False)
        t0 = time.perf_counter()
        for k in range(args.steps):
            tr._step(items[k], eps[k], 1.0, 1.0)
        tr.eng.read_losses(False)
        pipelined = (time.perf_counter() - t0) / args.steps * 1e3
        tr.close()
        res[f"hip_b{B}"] = {**summary(ts), "pipelined_ms_per_step": pipelined}
        xs = [torch.from_numpy(windows_of(seqs, items[k], perm)) for k in range(total)]
        rt = RefTrainer(init, num_training_steps=10 * total, dtype=torch.float32, device="cuda:0")
        ts = []
        for k in range(total):
            x, e = xs[k].cuda(), torch.from_numpy(eps[k]).cuda()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rt.step(x, e)   # the reference's .item() reads are part of its step
            torch.cuda.synchronize()
            if k >= args.warmup:
                ts.append(time.perf_counter() - t0)
        res[f"torch_gpu_b{B}"] = summary(ts)
        if not args.no_cpu:
            rt = RefTrainer(init, num_training_steps=10 * total, dtype=torch.float32, device="cpu")
            ts = []
            for k in range(2 + args.cpu_steps):
                t0 = time.perf_counter()
                rt.step(xs[k], torch.from_numpy(eps[k]))
                if k >= 2:
                    ts.append(time.perf_counter() - t0)
            res[f"torch_cpu{args.cpu_threads}_b{B}"] = summary(ts)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
