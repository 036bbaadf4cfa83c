"""Record the UNet launch schedules (tests/golden/unet_sched.json) that tests/test_gpu_unet_sched.py holds the engine to.

    python tests/golden/make_golden_sched.py [output.json [dump_dir]]          (on the MI355X)

For every case of CASES — a precision mode, a shape, said_debug_option settings — the file holds the stage list of Engine.profile_unet(reps=1)
(kind, epi, NB, KS, bytes, flops per launch, in launch order; the times are left out) and graph_num_nodes() after a one-step guided denoise_loop
of Be / 2 clips at the same frame count (run first).  Both depend on the host-side schedule alone (said_amd/csrc/unet_sched.cpp): record the file at the commit
whose schedule is to be kept, then change the schedule.  The script also prints which schedule functions each case went through.

With `dump_dir`, the UNet forward output and a 3-step guided denoise_loop result of every case (and of WIDE_BAND, whose alignment windows are wider
than said_profile_unet's S = T can make them) are saved there as <case>.pt for a bit-for-bit comparison between two builds (compare_dumps).
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from said_amd.util import synth  # noqa: E402

FIXTURE = os.path.join(HERE, "unet_sched.json")
TM = {"unet_tgemm_min_tokens": 0}   # every launch on the token-major GEMMs
CM = {"unet_tgemm_min_tokens": 1000000}   # ... on the channel-major ones

# name, precision, Be, T, cfg_clips, options
CASES = [
    ("fp32_default", "fp32", 2, 64, 0, {}),
    ("fp32_default_guided", "fp32", 2, 64, 1, {}),                              # sliced fused tail
    ("fp32_five_launch_tail", "fp32", 2, 64, 0, {"st_chain": 0}),
    ("fp32_five_launch_tail_guided", "fp32", 2, 64, 1, {"st_chain": 0}),
    ("fp32_token_major", "fp32", 2, 64, 0, TM),                                 # preparation kernels + token-major GEMM, the chain beside them
    ("fp32_token_major_guided", "fp32", 2, 64, 1, TM),
    ("fp32_token_major_out1", "fp32", 16, 704, 0, {**TM, "st_chain": 0}),       # 16 x 22 x 6 >= 2048 tile-heads: attn1.to_out token-major
    ("fp32_token_major_out1_guided", "fp32", 16, 704, 8, {**TM, "st_chain": 0}),
    ("bf16_default", "bf16", 2, 64, 0, {}),
    ("bf16_default_guided", "bf16", 2, 64, 1, {}),
    ("bf16_token_major", "bf16", 4, 96, 0, TM),                                 # the bf16 attention kernel, the fused bf16 tail
    ("bf16_token_major_guided", "bf16", 4, 96, 2, TM),
    ("bf16_token_major_long", "bf16", 2, 672, 0, TM),                           # T > 640: no bf16 attention kernel
    ("bf16_token_major_six_launch_tail", "bf16", 4, 96, 0, {**TM, "st_chain_bf16": 0}),          # the shared tail and proj_out's range split
    ("bf16_token_major_six_launch_tail_guided", "bf16", 4, 96, 2, {**TM, "st_chain_bf16": 0}),
    ("bf16_hybrid", "bf16", 4, 96, 0, {**TM, "tm_acts": 0}),
    ("bf16_hybrid_guided", "bf16", 4, 96, 2, {**TM, "tm_acts": 0}),
    ("bf16_hybrid_long", "bf16", 2, 672, 0, {**TM, "tm_acts": 0}),
    # 114 token tiles on the channel-major schedule: plan_gemm's NB 3 -> 2 fallback and kconv NB = 1 switch (the concatenated-input ResBlocks), multi-tile q/k/v
    ("fp32_long_two_samples", "fp32", 2, 1800, 0, {}),
    # ... and bf16 mode's multi-tile q/k/v and attn1.to_out; 3600 tokens are past the token-major threshold, so that is moved out of the way
    ("bf16_long_two_samples", "bf16", 2, 1800, 0, CM),
]
# S = 10 T: band_wmax > 8, the channel-major schedule's plain q projection + generic band kernel.  said_profile_unet runs S = T, so this
# branch has no stage list; it is covered by the bit-for-bit comparison alone.
WIDE_BAND = [("wide_band_fp32", "fp32", 2, 40, 400), ("wide_band_bf16", "bf16", 2, 40, 400), ("wide_band_bf16_token_major", "bf16", 2, 40, 400)]
FIELDS = ("kind", "epi", "NB", "KS", "bytes", "flops")   # of a stage, in the order the file lists them; the first four are integers
MC, FFI = 192, 768


def make_model(dev):
    from said_amd.model.diffusion import SAID_UNet1D
    from said_amd.model.wav2vec2 import AudioConfig
    m = SAID_UNet1D(audio_config=AudioConfig(num_hidden_layers=1))
    m.load_state_dict(synth.said_state_dict(num_w2v_layers=1), strict=True)
    return m.to(dev).eval()


class options:
    """The case's precision mode and debug options on the model's engine; both back to their defaults on exit."""

    def __init__(self, model, mode, Be, T, opts):
        self.model, self.mode, self.shape, self.opts = model, mode, (Be, T), opts

    def __enter__(self):
        self.model.set_mfma_dtype(self.mode)
        self.eng = self.model._get_engine(*self.shape)
        for k, v in self.opts.items():
            self.eng.debug_option(k, v)
        return self.eng

    def __exit__(self, *exc):
        for k in self.opts:
            self.eng.debug_option(k, -1)
        self.model.set_mfma_dtype("fp32")
        self.eng.set_precision("fp32")


def guided_loop(model, eng, dev, clips, T, steps):
    emb = synth.synth_latents(31, (clips, T, 768)).to(dev)
    lat = synth.synth_latents(32, (clips, T, 32)).to(dev)
    sch = model.noise_scheduler
    sch.set_timesteps(50)
    ts = sch.timesteps.numpy()
    coef = sch.coef_table(ts, 0.0)
    res, _, _ = eng.denoise_loop(latents=lat, context=emb, timesteps=ts[20:20 + steps], coef=coef[20:20 + steps], prediction_type="epsilon",
                                 guidance_scale=2.0, guidance_rescale=0.0, latent_scale=1.0)
    torch.cuda.synchronize()
    return res.cpu()


def record_case(model, dev, case):
    """{"stages": [...], "graph_nodes": n} of one case.  The loop runs first: it leaves the key-major K / V copy of this shape and precision behind, which
    the fused tails need — said_profile_unet computes no K / V, so without it the stage list would depend on the case that ran before."""
    name, mode, Be, T, cfg, opts = case
    with options(model, mode, Be, T, opts) as eng:
        guided_loop(model, eng, dev, Be // 2, T, 1)
        nodes = eng.graph_num_nodes()
        stages = [[s[k] for k in FIELDS] for s in eng.profile_unet(Be, T, reps=1, cfg_clips=cfg)]
        return {"stages": stages, "graph_nodes": nodes}


def functions_hit(case, stages):
    """Which schedule functions of unet_sched.cpp the stage list shows."""
    Be, T = case[2], case[3]
    stages = [dict(zip(FIELDS, s)) for s in stages]
    kinds = [s["kind"] for s in stages]
    nk = [round(s["flops"] / (2.0 * Be * T)) for s in stages]   # N x K of a launch over all Be samples
    x = [i for i, s in enumerate(stages) if s["kind"] in (6, 7)]
    hit = []
    if any(s["kind"] in (0, 2) and s["epi"] == 1 for s in stages) or (4 in kinds and not x) or any(s["kind"] in (0, 2) and s["epi"] == 3 for s in stages):
        hit.append("run_transformer")
    if x and 5 in kinds and any(s["kind"] == 4 and s["epi"] == 1 for s in stages):
        hit.append("run_transformer_hybrid")
    if any(s["kind"] in (6, 7) and s["epi"] == 1 for s in stages):
        hit.append("run_transformer_tm")
    if 9 in kinds:
        hit.append("battn")
    if 10 in kinds:
        hit.append("chain")
    if any(stages[i]["kind"] == 7 and nk[i] == MC * 2 * MC for i in x):   # the 1x1 skip convolution as a launch of its own
        hit.append("resblock_range_split")
    if any(stages[i]["kind"] == 7 and stages[i]["epi"] == 0 and nk[i] == MC * FFI for i in x):   # (P F2) h alone
        hit.append("proj_out_range_split")
    return hit


def dump_case(model, dev, case):
    name, mode, Be, T, cfg, opts = case
    with options(model, mode, Be, T, opts) as eng:
        x = synth.synth_latents(41, (Be, T, 32)).to(dev)
        c = synth.synth_latents(42, (Be, T, 768)).to(dev)
        ts = (torch.arange(Be) * 137 + 500) % 1000
        return {"forward": eng.unet_forward(x, ts, c).cpu(), "loop": guided_loop(model, eng, dev, max(Be // 2, 1), T, 3)}


def dump_wide(model, dev, case):
    name, mode, Be, T, S = case
    with options(model, mode, Be, T, TM if name.endswith("token_major") else {}) as eng:
        x = synth.synth_latents(43, (Be, T, 32)).to(dev)
        c = synth.synth_latents(44, (Be, S, 768)).to(dev)
        ts = (torch.arange(Be) * 137 + 500) % 1000
        return {"forward": eng.unet_forward(x, ts, c).cpu()}   # (the loop's context has one token per frame)


def compare_dumps(dir_a, dir_b):
    """Prints torch.equal of every tensor of every case; returns True when all are equal."""
    ok = True
    for f in sorted(os.listdir(dir_a)):
        a, b = torch.load(os.path.join(dir_a, f)), torch.load(os.path.join(dir_b, f))
        eq = {k: bool(torch.equal(a[k], b[k])) and bool(torch.isfinite(a[k]).all()) for k in a}
        ok = ok and all(eq.values())
        print(f"{f[:-3]:44s} " + "  ".join(f"{k}: {'equal' if v else 'DIFFERENT'}" for k, v in eq.items()))
    return ok


def main(out_path=FIXTURE, dump_dir=None):
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    model = make_model(dev)
    model._get_engine(16, 1800)   # the most samples and the most frames of any case: one workspace for all of them
    doc = {"comment": "recorded by tests/golden/make_golden_sched.py: launch order of said_profile_unet and graph nodes per guided step",
           "stage_fields": list(FIELDS), "cases": []}
    for case in CASES:
        rec = record_case(model, dev, case)
        hit = functions_hit(case, rec["stages"])
        print(f"{case[0]:44s} {case[1]} Be={case[2]} T={case[3]} cfg_clips={case[4]} {case[5]}: {len(rec['stages'])} launches, "
              f"{rec['graph_nodes']} graph nodes; " + ", ".join(hit), flush=True)
        doc["cases"].append({"name": case[0], "precision": case[1], "Be": case[2], "T": case[3], "cfg_clips": case[4], "options": case[5],
                             "functions": hit, **rec})
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("all functions hit:", sorted({h for c in doc["cases"] for h in c["functions"]}))
    if dump_dir:
        os.makedirs(dump_dir, exist_ok=True)
        for case in CASES:
            torch.save(dump_case(model, dev, case), os.path.join(dump_dir, case[0] + ".pt"))
        for case in WIDE_BAND:
            torch.save(dump_wide(model, dev, case), os.path.join(dump_dir, case[0] + ".pt"))
        print(f"dumped {len(CASES) + len(WIDE_BAND)} cases to {dump_dir}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
