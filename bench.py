"""bench.py — throughput of the SAiD denoising hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W            (N >= 1: spawns N ranks itself when not under torchrun)
    python bench.py --gpus 1 --steps K --warmup W --full     (the same run, then everything else the benchmark measures: see --full below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
    python bench.py --gpus 2 --dry_run_gloo                  (CPU: launch / shard / gather plumbing only, stand-in path)
    python bench.py --rccl_at_one                             (1 GPU: the RCCL collectives of the sharded run on a one-rank group)
    BASELINE configs[3] (8 GPUs, 256 clips): python bench.py --gpus 8 --batch 32 --steps 1 --warmup 1

One "step" = one pass of the hot path over one batch: Wav2Vec2 audio encode of B synthetic
10 s clips + `--num_steps` (1000) denoising steps of the conditional UNet1D with the CLI-default
classifier-free guidance + scheduler updates -> (B, 600, 32) blendshape coefficients (BASELINE.json
configs[1]).  Inputs (processed waveform, start noise) are resident in HBM before the timed region.
With N > 1 every rank processes its own B clips (weak scaling, no data-path collective) and one
RCCL all-gather assembles the (N*B, 600, 32) result, inside the timed region.

--dump-outputs DIR writes what the last timed step returned, (N*B, 600, 32) blendshape coefficients, as DIR/result.npy (float32;
above 64 MB a fixed seeded sample of the clips).  The inputs, the eta > 0 noise seed included, are the same in every pass and every
run with the same arguments, so two builds can be compared output for output.

Prints ONE JSON line (rank 0).  A plain run does what its headline figure needs and nothing else: set-up, warm-up, the timed steps,
--dump-outputs, the line.  --full measures, after the timed steps and the dump, what takes runs of its own, and attaches it to the line:
  roofline      dominant UNet kernel: algorithmic bytes per launch / HIP-event-timed launch duration (--no_roofline leaves it out)
  secondary     the other configurations of BASELINE.json, the strict-fp32 and the eta = 1 form of the headline, each with its own
                roofline (single-GPU headline run only; --no_secondary leaves them out)
  cpu_baseline  the CPU oracle (a port of the reference path, oracle/) timed on this host's cores on a
                bounded sample and extrapolated to the same workload (--no_cpu_baseline leaves it out)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MODES = {"f32": "fp32", "bf16": "bf16", "f32_strict": "fp32_strict"}   # --dtype -> SAID.set_mfma_dtype
DTYPE_LABEL = {"f32": "f32 (split-fp16 products)", "bf16": "bf16", "f32_strict": "f32"}   # the arithmetic the products run in (include/said_hip.h, said_set_precision)
HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 measured copy
# dense peaks of the matrix pipes (MI355X_MICROARCH.md); never the 2:1-sparsity figures.  A kernel is priced against the pipe its instructions run on.
PIPE_PEAK_TFLOPS = {"mfma_f32": 157.3, "mfma_f16": 2500.0, "mfma_bf16": 2500.0}
EPI_NAMES = {0: "store", 1: "qkv", 2: "geglu", 3: "band", -1: "attn"}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--batch", type=int, default=1, help="clips per GPU")
    p.add_argument("--seconds", type=float, default=10.0, help="clip length")
    p.add_argument("--num_steps", type=int, default=1000, help="denoising steps per clip")
    p.add_argument("--guidance_scale", type=float, default=2.0)
    p.add_argument("--eta", type=float, default=0.0)
    p.add_argument("--dtype", choices=["f32", "bf16", "f32_strict"], default="f32",
                   help="f32 (BASELINE configs[1]: fp32 tensors, products on split-fp16 operands), f32_strict (products on fp32 matrix instructions) or bf16 "
                        "multiplies with fp32 accumulation (configs[2]: --batch 32 --num_steps 50 --dtype bf16)")
    p.add_argument("--edit", action="store_true",
                   help="editing mode (BASELINE configs[4]: --seconds 30 --num_steps 100 --edit): init_samples + in-betweening mask "
                        "(middle third regenerated, 4 channels pinned), mask blend with the re-noised init every step")
    p.add_argument("--clip_groups", type=int, default=0,
                   help="0 (default): SAID.inference decides (SAID._pick_clip_groups: one group wherever the persistent GEMMs of round 4 fill "
                        "the chip on their own, two to four concurrent groups on their own streams otherwise); n >= 1: run every batch as n "
                        "concurrent clip groups (1: never split)")
    p.add_argument("--debug_option", action="append", default=[], metavar="NAME=VALUE",
                   help="development: said_debug_option(NAME, VALUE) on the engine before the first run (scripts/ A/B drivers)")
    p.add_argument("--ab_lib", default=None, metavar="PATH",
                   help="development: load this build of the library (scripts/build_variant.sh) instead of said_amd/lib/libsaid_hip.so; named in the JSON line")
    p.add_argument("--tm_acts", type=int, nargs="?", const=1, default=-1, choices=[-1, 0, 1],
                   help="large-batch schedule with token-major activations between the UNet kernels and the normalisations inside the consuming "
                        "GEMMs (41 launches per step): -1 (default) = on in bf16 mode, off in fp32 mode; 0 / 1 force it (said_debug_option tm_acts)")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps, write the result of the last one as DIR/result.npy (float32; at most 64 MB: a seeded sample of the clips above that)")
    p.add_argument("--full", action="store_true",
                   help="after the timed steps (and --dump-outputs), also measure what takes runs of its own and attach it to the line: the roofline "
                        "block, the secondary configurations and the CPU baseline (each with a --no_... switch); off by default: a plain run "
                        "sets up, warms up, times the steps and prints the line")
    p.add_argument("--no_cpu_baseline", action="store_true", help="with --full: leave the CPU baseline out")
    p.add_argument("--no_secondary", action="store_true",
                   help="with --full: skip the secondary configurations (BASELINE configs[2], [3] per GPU, [4], and the headline with eta = 1) that "
                        "the single-GPU headline run measures after the headline and attaches as `secondary`")
    p.add_argument("--no_roofline", action="store_true", help="with --full: leave the roofline block (and with it the secondary configurations) out")
    p.add_argument("--cpu_steps", type=int, default=40, help="UNet evaluations in the CPU-baseline sample")
    p.add_argument("--rccl_at_one", action="store_true",
                   help="N=1 only: create a ONE-rank 'nccl' (= RCCL) process group and run the sharded run's collectives on it")
    p.add_argument("--dry_run_fail_rank", type=int, default=-1, help="with --dry_run_gloo: the stand-in path raises on this rank (failure-handling test)")
    p.add_argument("--dry_run_gloo", action="store_true",
                   help="no GPU: run the launch / shard / all-gather / timing plumbing on CPU over gloo with a stand-in path")
    return p.parse_args()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """Write each (clips, ...) tensor of `arrays` as out_dir/<name>.npy in float32.  One above its share of `limit` keeps a sample of
    its clips drawn by numpy's default_rng(0), in clip order: the same rows in every run at the same shape.  Returns what was written."""
    fresh = not os.path.isdir(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    if fresh:   # a directory this creates ignores itself in git, wherever it is put (as .pytest_cache does)
        with open(os.path.join(out_dir, ".gitignore"), "w") as f:
            f.write("*\n")
    info = {}
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        n, cap = a.shape[0], max(1, limit // len(arrays) // (a[:1].nbytes or 1))
        rows = "all"
        if n > cap:
            a = a[np.sort(np.random.default_rng(0).choice(n, cap, replace=False))]
            rows = f"{cap} of {n} clips, sampled by numpy default_rng(0)"
        np.save(os.path.join(out_dir, name + ".npy"), a)
        info[name] = {"shape": list(a.shape), "dtype": "float32", "rows": rows}
    return info


def cpu_info():
    """(model name, physical cores, logical cpus) of this host from /proc/cpuinfo."""
    model, cores, logical = "unknown", set(), 0
    try:
        phys = core = None
        for ln in open("/proc/cpuinfo"):
            k, _, v = ln.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                model = v
            elif k == "processor":
                logical += 1
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
                cores.add((phys, core))
    except OSError:
        pass
    return model, (len(cores) or (os.cpu_count() or 1)), (logical or (os.cpu_count() or 1))


def cpu_baseline(args, T, Ta):
    """Oracle (CPU restatement of the reference path) on the host cores: one audio encode + a bounded
    number of CFG UNet steps + scheduler updates, extrapolated to num_steps."""
    from oracle import pipeline as op
    from oracle import scheduler as osch
    from oracle import unet as ou
    from said_amd.util import synth
    torch.set_grad_enabled(False)
    cpu_model, phys_cores, logical = cpu_info()
    avail = max(1, min(phys_cores, os.cpu_count() or 1))   # physical cores visible to this process
    cores = avail
    torch.set_num_threads(avail)
    sd = synth.said_state_dict()
    sd_a, sd_u, null = op.split_state_dict(sd)
    proc = op.process_audio(synth.synth_waveform(1234, Ta))
    t0 = time.perf_counter()
    emb = op.get_audio_embedding(sd_a, proc, T)
    t_audio = time.perf_counter() - t0
    do_cfg = args.guidance_scale > 1.0
    ctx = torch.cat([null.repeat(1, T, 1), emb]) if do_cfg else emb
    sch = osch.OracleDDIM()
    sch.set_timesteps(args.num_steps)
    lat = synth.synth_latents(0, (1, T, 32))
    n = max(2, args.cpu_steps)
    # thread count: this UNet is small (T = 600 tokens), so all physical cores is not necessarily the fastest setting (128
    # threads measured 2x slower than 64 on a 2 x 64-core host): time one evaluation at a few counts, keep the best — the
    # baseline should be the CPU at its best.  `cores` reports the threads actually used, `physical_cores` what the host has.
    xw = torch.cat([lat] * 2) if do_cfg else lat
    tw = sch.timesteps[:1].repeat(2 if do_cfg else 1)
    best = None
    for nt in sorted({avail, max(1, avail // 2), max(1, avail // 4), min(avail, 32), min(avail, 16), min(avail, 8)}, reverse=True):
        torch.set_num_threads(nt)
        ou.unet1d_forward(sd_u, xw, tw, ctx)  # warm
        t0 = time.perf_counter()
        ou.unet1d_forward(sd_u, xw, tw, ctx)
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, nt)
    cores = best[1]
    torch.set_num_threads(cores)
    ou.unet1d_forward(sd_u, xw, tw, ctx)  # warm
    t0 = time.perf_counter()
    done = 0
    for t in sch.timesteps[:n]:
        if done >= 3 and time.perf_counter() - t0 > 20.0:  # bounded sample: ~20 s of CPU work
            break
        done += 1
        x = torch.cat([lat] * 2) if do_cfg else lat
        pred = ou.unet1d_forward(sd_u, x, t.repeat(x.shape[0]), ctx)
        if do_cfg:
            e_u, e_c = pred.chunk(2)
            pred = e_c + args.guidance_scale * (e_c - e_u)
        lat = sch.step(pred, int(t), lat)
    n = done
    t_step = (time.perf_counter() - t0) / n
    total = t_audio + args.num_steps * t_step
    return {"value": round(T / total, 3), "unit": "frames/s", "cores": cores, "kind": "port",
            "cpu_model": cpu_model, "physical_cores": phys_cores, "logical_cpus": logical,
            "sample": f"1 clip: audio encode ({t_audio:.2f} s) + {n} of {args.num_steps} CFG UNet+scheduler steps "
                      f"({t_step * 1e3:.1f} ms each) on {cores} threads, extrapolated to {args.num_steps} steps",
            "clips_per_s": round(1.0 / total, 5)}


def source_hash():
    """sha256 (first 16 hex digits) over the kernel and engine sources: what a committed PMC traffic figure was measured on.
    (The GPU box has no .git; the sources identify the build.)"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "said_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h", ".cpp")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


# What a kernel's matrix products execute on, from its family name and the engine's arithmetic (include/said_hip.h, said_set_precision):
# fp32 mode multiplies on SPLIT-fp16 operands — three v_mfma_f32_32x32x16_f16 per k16 step where the fp32 matrix pipe would need eight
# v_mfma_f32_32x32x2_f32 — so its kernels' roof is the fp16 pipe (2.5 PFLOP/s dense) against the instructions they EXECUTE (3 x the
# fp32-equivalent flops), or equivalently 2500 / 3 = 833 TFLOP/s against fp32-equivalent flops.  VERDICT r5 #3: pricing fp32-equivalent
# flops against the fp32 pipe's 157.3 TFLOP/s gave "fractions" above 1.
def kernel_pipe(name, dtype, sp):
    """(pipe, executed MFMA flops per algorithmic flop) of a kernel family; pipe None: no matrix instructions."""
    fam = name.split("<")[0].split(" ")[0]
    if fam in ("prep_kernel",):
        return None, 0.0
    if dtype == "bf16":
        return "mfma_bf16", 1.0
    split = {"stchain_kernel": sp["chain"], "ugemm_kernel": sp["ugemm"], "out_conv": sp["ugemm"], "fgemm_kernel": sp["gemm"], "attn_kernel": sp["attn"], "attn2q_kernel": sp["attn"]}.get(fam, False)
    return ("mfma_f16", 3.0) if split else ("mfma_f32", 1.0)


def trace_name_prefix(name, dtype):
    """The rocprofv3 kernel-name prefix of a family label of roofline() (exact instantiation where the label carries it)."""
    epi_no = {v: k for k, v in EPI_NAMES.items()}
    fam = name.split("<")[0].split(" ")[0]
    args = name[name.index("<") + 1:name.rindex(">")].split(",") if "<" in name else []
    if fam == "stchain_kernel":   # stchain_kernel<bf16, slices>: every slice count of the precision mode
        return "said::stchain_kernel<" + ("true" if dtype == "bf16" else "false") + ","
    if fam == "attn_kernel" and len(args) == 2:
        return f"said::attn_kernel<{int(args[0][1:]) // 32}, {args[1][2:]},"
    if fam in ("ugemm_kernel", "cgemm_kernel") and len(args) == 3:
        return f"said::{fam}<{args[0][2:]}, {args[1][2:]}, {epi_no.get(args[2], 0)}" + ("," if fam == "ugemm_kernel" else ">")
    return "said::" + fam + ("<" if fam not in ("prep_kernel", "battn_kernel") else "")


def in_situ_from_trace(traffic_key, name, dtype):
    """(avg us, launches, file) of the family in the committed rocprofv3 kernel trace of this configuration — only when the trace was taken on the
    sources this run was built from (its `# source_hash=` header; scripts/gpu_r6_final.sh writes it), else None: a stale trace says nothing."""
    import re
    tfile = os.path.join(ROOT, "profiles", f"trace_latest_{traffic_key}.txt")
    if not os.path.exists(tfile):
        return None
    lines = open(tfile).read().splitlines()
    m = re.match(r"#\s*source_hash=(\w+)", lines[0]) if lines else None
    if not m or m.group(1) != source_hash():
        return None
    pre = trace_name_prefix(name, dtype)
    row = re.compile(r"^\s*([\d.]+)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+(.*)$")
    tot_us, calls = 0.0, 0
    for ln in lines:
        r = row.match(ln)
        if r and r.group(5).startswith(pre):
            tot_us += float(r.group(1)) * 1e3
            calls += int(r.group(2))
    return (tot_us / calls, calls, f"profiles/trace_latest_{traffic_key}.txt") if calls else None


def roofline(model, Be, T, step_ms, dtype, cfg_clips=0, traffic_key="cfg1", groups=1):
    """Per-kernel HIP-event timing of one UNet evaluation (said_profile_unet: every launch of the schedule replayed back to back in a graph on the
    caller's stream between two hipEvents) + the whole-step figures.  With clip groups (SAID.inference runs the batch as `groups` concurrent
    sub-batches) the launches are one GROUP's.

    Fractions (all <= 1 by construction):
      frac_hbm              algorithmic bytes of the launch (weights + operands in + residual + result out) / time / 8 TB/s
      frac_mfma_executed    matrix flops the kernel's instructions EXECUTE / time / the dense peak of the pipe they run on
      frac_fp32_equivalent  fp32-equivalent (algorithmic) flops / time / the rate at which that pipe delivers fp32-equivalent products (peak / 3 for
                            split-fp16 kernels); numerically equal to frac_mfma_executed, kept under the name earlier rounds reported
      frac                  the one of the roof that binds by arithmetic intensity (`bound`)
    Time: the in-situ average of a rocprofv3 trace taken on these very sources when profiles/ holds one, else the isolated replays (`time_source`)."""
    eng = model._eng
    B = cfg_clips if cfg_clips else Be
    per = Be // B                                    # UNet samples per clip (2 under guidance)
    sizes = [B * (i + 1) // groups - B * i // groups for i in range(groups)]
    nmax = max(sizes)
    stages = eng.profile_unet(per * nmax, T, reps=40, cfg_clips=nmax if cfg_clips else 0)
    sp = dict(attn=False, gemm=False, ugemm=False, chain=False)
    if dtype in ("f32", "f32_strict"):
        for k, opt in (("attn", "attn_split"), ("gemm", "gemm_split"), ("ugemm", "ugemm_split"), ("chain", "st_chain")):
            try:
                sp[k] = eng.debug_get(opt) == 1
            except Exception:
                pass
    agg = {}
    for st in stages:
        name = ("attn2q_kernel<4, 3>" if st["kind"] == 1 and st["KS"] == 34 else   # (three query tiles per wave: attn2q.hip)
                f"attn_kernel<D{32 * st['NB']},KS{st['KS']}>" if st["kind"] == 1 else
                "battn_kernel" if st["kind"] == 9 else
                f"{'fgemm' if st['KS'] == 32 else 'tgemm'}_kernel<{st['NB']},{EPI_NAMES[st['epi']]}>" if st["kind"] == 4 else
                "prep_kernel" if st["kind"] == 5 else
                f"xgemm_kernel<{st['NB']},{'f32' if st['KS'] == 32 else 'bf16'},{EPI_NAMES[st['epi']]}>" if st["kind"] == 6 else
                f"rgemm_kernel<{EPI_NAMES[st['epi']]}>" if st["kind"] == 7 else
                "stchain_kernel" if st["kind"] == 10 else
                "conv_in_kernel" if st["kind"] == 11 else
                "out_conv (ugemm_kernel<NB1,KS8,store>; in the loop: first half of out_sched_kernel)" if st["kind"] == 12 else
                f"{'ugemm' if st['kind'] == 2 else 'cgemm'}_kernel<NB{st['NB']},KS{st['KS']},{EPI_NAMES[st['epi']]}>")
        a = agg.setdefault(name, dict(us=0.0, bytes=0.0, flops=0.0, launches=0))
        a["us"] += st["us"]; a["bytes"] += st["bytes"]; a["flops"] += st["flops"]; a["launches"] += 1
    for name, a in agg.items():
        a["pipe"], a["mult"] = kernel_pipe(name, "bf16" if dtype == "bf16" else "f32", sp)
    dom = max(agg, key=lambda k: agg[k]["us"])
    d = agg[dom]
    t_iso = d["us"] / d["launches"]
    situ = in_situ_from_trace(traffic_key, dom, dtype) if groups == 1 else None
    t_us = situ[0] if situ else t_iso
    bytes_l, flops_l = d["bytes"] / d["launches"], d["flops"] / d["launches"]
    pipe_peak = PIPE_PEAK_TFLOPS[d["pipe"]] if d["pipe"] else None
    gbs = bytes_l / (t_us * 1e-6) / 1e9
    tf_alg = flops_l / (t_us * 1e-6) / 1e12
    tf_exec = tf_alg * d["mult"]
    frac_hbm = gbs / HBM_PEAK_GBS
    frac_exec = tf_exec / pipe_peak if pipe_peak else 0.0
    mfma_bound = bool(pipe_peak) and (flops_l * d["mult"] / max(bytes_l, 1.0)) > pipe_peak * 1e12 / (HBM_PEAK_GBS * 1e9)
    from said_amd import _engine
    # SURVEY 8(d)'s byte model at the element size the schedule stores between its kernels: bf16 where the token-major-activation kernels run, fp32 elsewhere
    tm_acts = any(st["kind"] in (6, 7, 8) for st in stages)
    elem = 2 if (dtype == "bf16" and tm_acts) else 4
    unet_bytes = _engine.unet_algorithmic_bytes(Be, T, elem)
    unet_flops = _engine.unet_algorithmic_flops(Be, T)
    sum_us = sum(a["us"] for a in agg.values())
    # the whole step against the matrix pipes: the time the pipes would need at their dense peaks for the instructions the schedule executes (per family:
    # executed flops / its pipe's peak) over the loop's step time.  Under guidance the shared prefix runs once per clip, so executed < reference-equivalent work.
    t_pipes_us = 0.0
    exec_flops = exec_bytes = 0.0
    for n in sorted(set(sizes)):
        st_n = stages if n == nmax else eng.profile_unet(per * n, T, reps=1, cfg_clips=n if cfg_clips else 0)
        exec_flops += sizes.count(n) * sum(st["flops"] for st in st_n)
        exec_bytes += sizes.count(n) * sum(st["bytes"] for st in st_n)
    for a in agg.values():
        if a["pipe"]:
            t_pipes_us += (sum(sizes) / nmax) * a["flops"] * a["mult"] / (PIPE_PEAK_TFLOPS[a["pipe"]] * 1e12) * 1e6   # (agg is ONE group of nmax clips)
    arith = ("bf16 operands (v_mfma_f32_32x32x16_bf16), fp32 accumulation" if dtype == "bf16" else
             "split-fp16 operands (x = h + 2^-11 l; three v_mfma_f32_32x32x16_f16 per k16 step), fp32 accumulation" if d["pipe"] == "mfma_f16" else
             "fp32 operands (v_mfma_f32_32x32x2_f32)" if d["pipe"] else "no matrix instructions")
    out = {"bound": "mfma" if mfma_bound else "hbm", "kernel": dom,
           "achieved": round(tf_exec, 3) if mfma_bound else round(gbs, 2), "peak": pipe_peak if mfma_bound else HBM_PEAK_GBS,
           "unit": "TFLOP/s" if mfma_bound else "GB/s",
           "frac": round(frac_exec if mfma_bound else frac_hbm, 5),
           "frac_hbm": round(frac_hbm, 5), "frac_mfma_executed": round(frac_exec, 5), "frac_fp32_equivalent": round(frac_exec, 5),
           "fp32_equivalent_peak_tflops": round(pipe_peak / d["mult"], 1) if pipe_peak and d["mult"] else None,
           "kernel_arithmetic": arith, "pipe": d["pipe"], "executed_flops_per_algorithmic_flop": d["mult"],
           "arithmetic_intensity_executed": round(flops_l * d["mult"] / max(bytes_l, 1.0), 1),
           "hbm_GBps": round(gbs, 2), "traffic": None, "traffic_source": None,
           "launches_per_unet": d["launches"], "avg_launch_us": round(t_us, 3), "time_source": (f"in situ: {situ[2]} ({situ[1]} launches, same source hash)" if situ else
                                                                                              "isolated replays (HIP events around 40 back-to-back launches per stage, this run)"),
           "avg_launch_us_isolated": round(t_iso, 3),
           "alg_bytes_per_launch": round(bytes_l), "alg_gflop_per_launch": round(flops_l / 1e9, 4),
           "kernel_tflops_fp32_equivalent": round(tf_alg, 3), "kernel_tflops_executed": round(tf_exec, 3),
           "clip_groups": groups, "launch_unet_batch": per * nmax,
           "unet_step": {"ms_loop_per_step": round(step_ms, 4), "sum_kernel_us_isolated": round(sum_us, 2), "launches": len(stages) * groups,
                         "alg_bytes": round(unet_bytes), "alg_gflop": round(unet_flops / 1e9, 3), "alg_bytes_elem_size": elem,
                         "hbm_frac": round(unet_bytes / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                         "hbm_frac_is": "SURVEY 8(d) algorithmic bytes of the full UNet batch / loop time per step / 8 TB/s (north_star bar: 0.40)",
                         "mfma_frac_executed": round(t_pipes_us / (step_ms * 1e3), 5),
                         "mfma_frac_executed_is": "time the matrix pipes need at dense peak for the instructions the schedule executes / loop time per step",
                         "executed_gflop_fp32_equivalent": round(exec_flops / 1e9, 3), "executed_bytes_per_launch_sum": round(exec_bytes)},
           "by_kernel": {k: {"us": round(v["us"], 2), "launches": v["launches"], "pipe": v["pipe"],
                             "frac_hbm": round(v["bytes"] / (v["us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                             "frac_mfma_executed": round(v["flops"] * v["mult"] / (v["us"] * 1e-6) / 1e12 / PIPE_PEAK_TFLOPS[v["pipe"]], 4) if v["pipe"] else 0.0}
                         for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["us"])}}
    # Two byte models: `frac_hbm` prices the family's PER-LAUNCH operand bytes; `hbm_frac_8d` its share of SURVEY 8(d)'s whole-UNet bytes
    # (an activation counted once however many launches touch it), apportioned by the family's share of the per-launch bytes.
    tot_launch_bytes = sum(a["bytes"] for a in agg.values())
    if tot_launch_bytes > 0:
        out["alg_bytes_8d_share"] = round(unet_bytes * d["bytes"] / tot_launch_bytes)
        out["hbm_frac_8d"] = round(unet_bytes * d["bytes"] / tot_launch_bytes / (t_us * d["launches"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 5)
    out["precision_mode"] = eng.effective_precision()
    out["fp32_products"] = {"attention": "split_fp16" if sp["attn"] else "mfma_f32", "small_batch_gemms": "split_fp16 (ugemm_kernel SP)" if sp["ugemm"] else "mfma_f32",
                            "transformer_tail": "stchain_kernel (split_fp16)" if sp["chain"] else "five launches", "large_batch_gemms": "split_fp16 (fgemm_kernel SP)" if sp["gemm"] else "mfma_f32"} if dtype != "bf16" else None
    if sum_us > 0 and groups == 1:   # (concurrent clip groups share the chip: a launch's in-situ time is then not comparable with its isolated one)
        out["in_situ_scale"] = round((step_ms * 1e3) / sum_us, 4)   # loop time per step / sum of the isolated launch times (includes the ~1.8 us per graph node between kernels)
    # HBM traffic from the PMC counters is collected in its own rocprofv3 passes (scripts/gpu_r3_traffic.sh; --pmc must not be combined with tracing) and
    # committed: it is NOT measured in this run, hence the explicit source label and the staleness flag
    tf = os.path.join(ROOT, "profiles", "traffic_latest.json")
    if os.path.exists(tf):
        try:
            tr = json.load(open(tf)).get("configs", {}).get(traffic_key)
            if tr and tr.get("kernel") == dom:
                out["traffic"] = tr.get("hbm_bytes_per_launch")
                out["traffic_source"] = "profiles/traffic_latest.json[" + traffic_key + "] (" + str(tr.get("source", "separate rocprofv3 --pmc passes")) + ")"
                out["traffic_stale"] = tr.get("source_hash") != source_hash()
                out["traffic_git_sha"] = tr.get("git_sha")
        except Exception:
            pass
    return out


def audio_encode_block(model, proc, T, B, dtype):
    """Audio encoder alone (once per clip): HIP-event time of get_audio_embedding on the current stream."""
    model.get_audio_embedding(proc, T)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 3
    ev0.record()
    for _ in range(reps):
        model.get_audio_embedding(proc, T)
    ev1.record()
    torch.cuda.synchronize()
    ms = ev0.elapsed_time(ev1) / reps
    Ta = proc.shape[1]
    # conv stack 24.56 GMAC (at 160,000 samples, scales with Ta), projection 0.39 MMAC/frame, pos-conv
    # 4.72 MMAC/frame, 12 layers x (7.08 MMAC/frame + 2*768*T MAC/frame of attention)
    mac = 24.56e9 * Ta / 160000.0 + T * (0.393e6 + 4.719e6 + 12 * (7.078e6 + 2 * 768.0 * T))
    weights_b = 94371712 * 4.0
    act_b = 512 * ((Ta - 10) // 5 + 1) * 4.0 * 2     # conv0 activation written + read once per clip
    return {"ms_per_clip": round(ms / B, 4), "ms_per_batch": round(ms, 3), "clips": B,
            "tflops": round(2 * mac * B / (ms * 1e-3) / 1e12, 2),
            "mfma_dtype": dtype, "mfma_frac": round(2 * mac * B / (ms * 1e-3) / 1e12 / PIPE_PEAK_TFLOPS["mfma_bf16" if dtype == "bf16" else "mfma_f32"], 4),
            "mfma_frac_is": "fp32-equivalent flops against the bf16 pipe (bf16 mode) / the fp32 pipe (fp32 modes: the encoder's GEMMs run on v_mfma_f32_32x32x2_f32; only its attention products are split-fp16)",
            "alg_bytes": round(weights_b + B * act_b), "alg_GBps": round((weights_b + B * act_b) / (ms * 1e-3) / 1e9, 1)}



def make_inputs(model, dev, clips, seconds, edit):
    """Synthetic inputs of SURVEY.md 8d for the given GLOBAL clip ids, resident in HBM: processed waveform, start latents, and
    (editing) init_samples = sigmoid(randn) * 0.5 with the in-betweening mask (outer thirds kept, channels 0-3 pinned)."""
    from said_amd.util import synth
    Ta = int(round(seconds * 16000))
    T = int(Ta / 16000 * 60)
    wav = [synth.synth_waveform(c, Ta).numpy() for c in clips]
    proc = model.process_audio(wav).to(dev)
    lat0 = torch.cat([synth.synth_latents(c, (1, T, 32)) for c in clips]).to(dev)
    edit_kw = {}
    if edit:
        B = len(clips)
        init_samples = (torch.sigmoid(torch.cat([synth.synth_latents(1000 + c, (1, T, 32)) for c in clips])) * 0.5).to(dev)
        mask = torch.zeros(B, T, 32, device=dev)
        mask[:, : T // 3] = 1.0
        mask[:, 2 * T // 3:] = 1.0
        mask[:, :, :4] = 1.0
        edit_kw = dict(init_samples=init_samples, mask=mask, edit_noise=lat0)
    return proc, lat0, edit_kw, T, Ta


def loop_step_ms(model, proc, lat0, edit_kw, T, num_steps, gs, eta):
    """Denoising loop alone (audio embedding precomputed), HIP events on the stream the engine launches on: ms per step."""
    emb = model.get_audio_embedding(proc, T)
    n = min(num_steps, 200)
    # (untimed first: the SAME step count — the step graphs are captured per schedule length, and with 50 steps per graph a capture inside the timed call would be ~8 % of it)
    model.inference(proc, num_inference_steps=n, guidance_scale=gs, eta=eta, init_latents=lat0, audio_embedding=emb, **edit_kw)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    model.inference(proc, num_inference_steps=n, guidance_scale=gs, eta=eta, init_latents=lat0, audio_embedding=emb, **edit_kw)
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / n


# Secondary configurations measured by the single-GPU headline run with --full (after the headline; N = 1 only).  Each is
# `python bench.py <flags>` in its own right; here they run for `passes` timed passes after one short warm-up pass.
SECONDARY = {
    "cfg2_bf16": dict(batch=32, seconds=10.0, num_steps=50, dtype="bf16", eta=0.0, edit=False, passes=2,
                      flags="--batch 32 --num_steps 50 --dtype bf16",
                      workload="BASELINE.json configs[2]: 32 clips x 10 s (T=600), audio encode + 50 DDIM steps, guidance 2 (UNet batch 64), bf16 mode"),
    "cfg3_per_gpu_f32": dict(batch=32, seconds=10.0, num_steps=1000, dtype="f32", eta=0.0, edit=False, passes=1,
                             flags="--batch 32 --steps 1 --warmup 1",
                             workload="BASELINE.json configs[3], ONE GPU's share: 32 clips x 10 s, audio encode + 1000 DDIM steps, guidance 2, fp32 (no all-gather at N = 1)"),
    "cfg3_one_group": dict(batch=32, seconds=10.0, num_steps=1000, dtype="f32", eta=0.0, edit=False, passes=1, clip_groups=1,
                           flags="--batch 32 --steps 1 --warmup 1 --clip_groups 1",
                           workload="configs[3]'s per-GPU share as ONE clip group (the default runs three concurrent groups: DESIGN.md 5)"),
    "cfg4_edit": dict(batch=1, seconds=30.0, num_steps=100, dtype="f32", eta=0.0, edit=True, passes=2,
                      flags="--seconds 30 --num_steps 100 --edit",
                      workload="BASELINE.json configs[4]: editing mode, 1 clip x 30 s (T=1800), init_samples + in-betweening mask, 100 DDIM steps, guidance 2, fp32"),
    "cfg1_strict_fp32": dict(batch=1, seconds=10.0, num_steps=1000, dtype="f32_strict", eta=0.0, edit=False, passes=2,
                             flags="--dtype f32_strict",
                             workload="BASELINE.json configs[1] in SAID_PREC_FP32_STRICT: every product on v_mfma_f32_32x32x2_f32 with fp32 operands (the price of true fp32 matrix instructions; the transformer tail as five launches)"),
    "cfg1_eta1": dict(batch=1, seconds=10.0, num_steps=1000, dtype="f32", eta=1.0, edit=False, passes=2,
                      flags="--eta 1",
                      workload="BASELINE.json configs[1] with eta = 1 (ancestral / DDPM-variance sampling, noise generated in the step's last kernel): 1 clip x 10 s, 1000 steps, guidance 2, fp32"),
}


def run_secondary(model, dev, gs):
    """The secondary configurations on the SAME model object (its engine workspace grows; the weights are uploaded once)."""
    out = {}
    for name, c in SECONDARY.items():
        B = c["batch"]
        proc, lat0, edit_kw, T, Ta = make_inputs(model, dev, range(B), c["seconds"], c["edit"])
        model.set_mfma_dtype(MODES[c["dtype"]])
        model.clip_groups = c.get("clip_groups")
        for k, v in c.get("debug", {}).items():
            model._get_engine(2 * B if gs > 1.0 else B, T).debug_option(k, v)

        def one(n_steps):
            return model.inference(proc, num_inference_steps=n_steps, guidance_scale=gs, eta=c["eta"], init_latents=lat0, **edit_kw).result

        one(c["num_steps"] if c["num_steps"] >= 400 else min(c["num_steps"], 10))   # warm-up: workspace growth, graph capture (long loops: 50 steps per graph — the real length; short ones: 10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(c["passes"]):
            res = one(c["num_steps"])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / c["passes"]
        assert torch.isfinite(res).all()
        Be = 2 * B if gs > 1.0 else B
        step_ms = loop_step_ms(model, proc, lat0, edit_kw, T, c["num_steps"], gs, c["eta"])
        rf = roofline(model, Be, T, step_ms, c["dtype"], cfg_clips=B if gs > 1.0 else 0, traffic_key="cfg1" if name == "cfg1_eta1" else "cfg1_strict" if name == "cfg1_strict_fp32" else ("cfg3_per_gpu_f32" if name == "cfg3_per_gpu_f32" else name),   # (eta = 1 runs the headline's kernels)
                      groups=model._pick_clip_groups(B, Be // B * T))
        rf["audio_encode"] = audio_encode_block(model, proc, T, B, c["dtype"])
        rf.pop("by_kernel", None)      # the headline's roofline carries the per-kernel table; keep the line readable
        out[name] = {"value": round(B * T / dt, 2), "unit": "frames/s", "ms_per_step": round(dt * 1e3, 3), "passes": c["passes"],
                     "clips_per_s": round(B / dt, 4), "realtime_factor": round(B * T / dt / 60.0, 2),
                     "ms_per_denoise_step": round(step_ms, 4), "dtype": DTYPE_LABEL[c["dtype"]], "workload": c["workload"],
                     "command": "python bench.py " + c["flags"], "graph_nodes_per_step": model._eng.graph_num_nodes(), "roofline": rf,
                     "clip_groups": model._pick_clip_groups(B, Be // B * T)}
        for k in c.get("debug", {}):
            model._eng.debug_option(k, -1)
        model.clip_groups = None
    model.set_mfma_dtype("fp32")
    return out


def run(args):
    """One rank of the bench (rank / world from the torchrun-style environment)."""
    from said_amd import shard
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    B, Ta = args.batch, int(round(args.seconds * 16000))
    T = int(Ta / 16000 * 60)
    torch.set_grad_enabled(False)

    if args.dry_run_gloo:
        # plumbing only: same launch, shard, gather and timing code, CPU stand-in for the path (no HIP, no numbers)
        dist = shard.init_process_group("gloo", rank, world) if world > 1 else None

        def path_fn(clips):
            if rank == args.dry_run_fail_rank:
                raise RuntimeError(f"stand-in path failure on rank {rank}")
            return torch.stack([torch.full((T, 32), float(c)) for c in clips])

        r = shard.timed_sharded_passes(path_fn, rank=rank, world=world, clips_per_rank=B, steps=args.steps, warmup=args.warmup,
                                       dist=dist, device=torch.device("cpu"))
        if rank == 0:
            want = sum(float(c) * T * 32 for c in range(world * B))
            line = {"dry_run": "gloo/cpu stand-in path: NOT a measurement", "n_gpus": world, "steps": args.steps,
                    "warmup": args.warmup, "clip_ranges": r.clip_ranges, "gathered_shape": list(r.gathered.shape),
                    "gathered_checksum": r.checksum, "checksum_ok": r.checksum == want}
            if args.dump_outputs:
                line["dump_outputs"] = {"dir": args.dump_outputs, "arrays": dump_outputs(args.dump_outputs, {"result": r.gathered})}
            print(json.dumps(line), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: said_amd has no CPU path (use --dry_run_gloo for the launch plumbing)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if args.rccl_at_one and world == 1:
        os.environ.setdefault("MASTER_PORT", str(shard.free_port()))
    # "nccl" IS RCCL on ROCm.  --rccl_at_one: a one-rank process group, so that the collectives of the sharded run (all-gather,
    # barriers, max-reduce of the time) execute on RCCL on a single-GPU box as well
    dist = shard.init_process_group("nccl", rank, world, dev) if (world > 1 or args.rccl_at_one) else None

    if dist is not None:
        # one process per GPU, really: a mis-launch (two ranks on one device) must not be able to report an N-GPU number from fewer GPUs
        pr = torch.cuda.get_device_properties(dev)
        ident = "|".join(str(getattr(pr, k, "?")) for k in ("uuid", "pci_domain_id", "pci_bus_id", "pci_device_id")) + f"|visible#{local}|{os.environ.get('HIP_VISIBLE_DEVICES', '')}"
        idents = [None] * world
        dist.all_gather_object(idents, ident)
        if len(set(idents)) != dist.get_world_size() or dist.get_world_size() != args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: {dist.get_world_size()} ranks on {len(set(idents))} distinct devices: {idents}")

    t_start = time.perf_counter()
    if args.ab_lib:
        from said_amd import _engine
        _engine._LIB_PATH = os.path.abspath(args.ab_lib)
    from said_amd.model.diffusion import SAID_UNet1D
    from said_amd.util import synth
    model = SAID_UNet1D()
    model.load_state_dict(synth.said_state_dict(), strict=True)
    model.to(dev).eval()
    torch.cuda.synchronize(dev)
    t_model = time.perf_counter()
    model.set_mfma_dtype(MODES[args.dtype])
    model.clip_groups = args.clip_groups or None
    for kv in args.debug_option:
        k, v = kv.split("=")
        model._get_engine(2 * B if args.guidance_scale > 1.0 else B, T).debug_option(k, int(v))
    if args.tm_acts >= 0:
        model._get_engine(2 * B if args.guidance_scale > 1.0 else B, T).debug_option("tm_acts", args.tm_acts)
    # synthetic inputs, resident in HBM before the timed region; keyed by GLOBAL clip id
    clips = shard.clip_range(rank, world, B)
    proc, lat0, edit_kw, T, Ta = make_inputs(model, dev, clips, args.seconds, args.edit)

    def path_fn(_clips):
        torch.default_generator.manual_seed(0)   # SAID.inference draws the eta > 0 noise seed on torch's CPU generator: the same one in every pass and run
        return model.inference(proc, num_inference_steps=args.num_steps, guidance_scale=args.guidance_scale, eta=args.eta,
                               init_latents=lat0, **edit_kw).result

    # Per-rank start-up, outside the timed passes and reported beside them: the first call creates the engine context, packs and uploads the
    # weights (101 M packed parameters), encodes the audio once and captures the step graph (which does not depend on the step count: ten steps suffice).
    model.inference(proc, num_inference_steps=min(args.num_steps, 10), guidance_scale=args.guidance_scale, eta=args.eta, init_latents=lat0, **edit_kw)
    torch.cuda.synchronize(dev)
    t_ready = time.perf_counter()
    startup = [t_model - t_start, t_ready - t_model]
    if dist is not None:
        st = torch.tensor(startup, device=dev, dtype=torch.float64)
        dist.all_reduce(st, op=dist.ReduceOp.MAX)
        startup = st.tolist()

    r = shard.timed_sharded_passes(path_fn, rank=rank, world=world, clips_per_rank=B, steps=args.steps, warmup=args.warmup,
                                   dist=dist, device=dev)
    elapsed = r.elapsed_s
    assert torch.isfinite(r.gathered).all()
    # copied out before anything below runs the model again
    dumped = dump_outputs(args.dump_outputs, {"result": r.gathered}) if (args.dump_outputs and rank == 0) else None

    if rank == 0:
        frames = world * B * T * args.steps
        Be = 2 * B if args.guidance_scale > 1.0 else B
        line = {
            "metric": "blendshape frames/sec (and clips/sec) at 1000 DDPM steps, 10 s audio",
            "value": round(frames / elapsed, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": DTYPE_LABEL[args.dtype], "data": "synthetic",
            "clips_per_s": round(world * B * args.steps / elapsed, 4),
            "realtime_factor": round(frames / elapsed / 60.0, 2),
            "startup_s": {"model_build_and_to_device": round(startup[0], 3), "engine_create_weight_pack_upload_first_encode_graph_capture": round(startup[1], 3),
                          "note": "max over ranks; outside the timed passes (once per process, not per pass)"},
            "config": {"workload": f"{B} clip(s)/GPU x {args.seconds:g} s synthetic audio (T={T} frames), audio encode + "
                                   f"{args.num_steps} DDIM steps (eta={args.eta:g}), guidance_scale={args.guidance_scale:g} "
                                   f"(UNet batch {Be}), " + ("editing mode: init_samples + in-betweening mask; " if args.edit else "") + ("fp32 tensors, products on split-fp16 operands (22-bit significands, fp32 accumulation); BASELINE.json configs[1]" if args.dtype == "f32" else
                                                              "strict fp32 (fp32 matrix instructions); BASELINE.json configs[1]" if args.dtype == "f32_strict" else
                                                              "bf16 mode (UNet: bf16 multiplies, fp32 accumulation and storage; audio encoder: bf16 GEMM operands and activations, fp32 residual stream); BASELINE.json configs[2] shape"),
                       "batch_per_gpu": B, "frames": T, "num_steps": args.num_steps, "guidance_scale": args.guidance_scale,
                       "eta": args.eta, "parallelism": f"clips sharded over {world} GPU(s), one RCCL all-gather" if world > 1 else ("single GPU, one-rank RCCL group (all-gather + barriers executed)" if dist is not None else "single GPU"),
                       "clip_ranges": r.clip_ranges, "gathered_checksum": r.checksum,
                       "graph_nodes_per_step": model._eng.graph_num_nodes()},
        }
        if dumped is not None:
            line["dump_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        if args.ab_lib or args.debug_option:
            line["development_build"] = {"ab_lib": args.ab_lib, "debug_option": args.debug_option}   # not the shipped defaults: an A/B run
        if args.full and not args.no_roofline:
            step_ms = loop_step_ms(model, proc, lat0, edit_kw, T, args.num_steps, args.guidance_scale, args.eta)
            headline = (B == 1 and args.seconds == 10.0 and args.num_steps == 1000 and args.dtype == "f32" and not args.edit and args.eta == 0.0)
            key = ("cfg1" if headline else
                   "cfg2_bf16" if (B == 32 and args.num_steps == 50 and args.dtype == "bf16") else
                   "cfg3_per_gpu_f32" if (B == 32 and args.dtype == "f32" and not args.edit) else
                   "cfg4_edit" if args.edit else "other")
            line["roofline"] = roofline(model, Be, T, step_ms, args.dtype, cfg_clips=B if args.guidance_scale > 1.0 else 0, traffic_key=key,
                                        groups=model._pick_clip_groups(B, Be // B * T))
            line["roofline"]["audio_encode"] = audio_encode_block(model, proc, T, B, args.dtype)
            if headline and world == 1 and not args.no_secondary:
                line["secondary"] = run_secondary(model, dev, args.guidance_scale)
                # the same figures as flat numeric top-level keys (a parser that keeps only scalars of the line still sees them)
                for name, sec in line["secondary"].items():
                    line[name + "_value"] = sec["value"]
                    line[name + "_ms_per_denoise_step"] = sec["ms_per_denoise_step"]
                    line[name + "_clip_groups"] = sec["clip_groups"]
                    rf = sec.get("roofline") or {}
                    if rf:   # the configuration's own roofline figures (dominant kernel family against the roof that binds it)
                        line[name + "_roofline_frac"] = rf.get("frac")
                        line[name + "_roofline_bound"] = rf.get("bound")
                        line[name + "_hbm_frac_step"] = (rf.get("unet_step") or {}).get("hbm_frac")
                        line[name + "_mfma_frac_executed_step"] = (rf.get("unet_step") or {}).get("mfma_frac_executed")
        if args.full and not args.no_cpu_baseline and world == 1:   # reported at N=1 only: other ranks would sit in the final barrier
            line["cpu_baseline"] = cpu_baseline(args, T, Ta)
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def main():
    args = parse()
    if args.gpus < 1:
        raise SystemExit(f"--gpus {args.gpus}: need at least one GPU")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit(f"--steps {args.steps} --warmup {args.warmup}: need at least one timed step and no negative warm-up")
    if not args.dry_run_gloo:
        # fail fast, before any rank is spawned: one process per GPU, HIP_VISIBLE_DEVICES (if set) already narrowed the
        # devices this process sees, and rank r uses visible device LOCAL_RANK = r
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} MI355X device(s) visible to this process "
                             f"(HIP_VISIBLE_DEVICES={os.environ.get('HIP_VISIBLE_DEVICES', '<unset>')}); said_amd has no CPU path "
                             "(--dry_run_gloo exercises the launch plumbing on CPU)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started as a plain `python bench.py --gpus N`: launch the N ranks here (one process per GPU)
        from said_amd import shard
        shard.spawn(run, (args,), args.gpus)
        return
    run(args)


if __name__ == "__main__":
    main()
