"""Generate golden G14 (tests/golden/g14_vae_train.npz): 20 training steps of the reference BCVAE.

Runs only where the reference checkout is present (never on the GPU box).  said/model/vae.py is loaded by file path (said/__init__.py imports
librosa).  After torch.manual_seed(0) the reference BCVAE() gives the initial state; eight seeded synthetic sequences, the windows of 20
batches of 8 (sequence, bdx, flip, zero) and the noise of each step are fixed.  Each step is script/train_vae.py's: the reference module's
forward with that noise, elbo_loss (no std), backward, torch's clip_grad_norm_(1.0) and AdamW(lr=1e-4), diffusers' EMA (decay 0.99, restated)
and constant_with_warmup over 20 training steps (restated); once in float32 and once in float64.  Stored: the 20 x 4 losses of both runs,
the step-1 gradients, and the final parameters, running statistics and EMA shadow of the float64 run; tensors above 512 elements as 256
evenly spaced entries (subset_index) plus their sum and sum of squares.  The reference's class list, mirror pairs and person-ID splits
(script/dataset/dataset_voca.py) are stored as text.

Usage:  python tests/golden/make_golden_g14.py
"""
import ast
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference"
STEPS, BATCH, LR = 20, 8, 1e-4
FULL_MAX, SUBSET = 512, 256   # keeps the file small: tensors above FULL_MAX elements are stored as SUBSET evenly spaced entries

from said_amd.util.scheduler import constant_with_warmup_lambda, ema_decay  # noqa: E402
from vae_train_ref import elbo, windows_of  # noqa: E402


def reference_lists():
    tree = ast.parse(open(os.path.join(REF, "script/dataset/dataset_voca.py")).read())
    out = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and node.name == "BlendVOCADataset":
            for st in node.body:
                if isinstance(st, ast.Assign) and isinstance(st.targets[0], ast.Name):
                    name = st.targets[0].id
                    if name in ("person_ids_train", "person_ids_val", "person_ids_test", "default_blendshape_classes",
                                "default_blendshape_classes_mirror_pair"):
                        out[name] = ast.literal_eval(st.value)
    return out


def load_reference_vae():
    spec = importlib.util.spec_from_file_location("ref_vae", os.path.join(REF, "said/model/vae.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def subset_index(size: int) -> np.ndarray:
    """The entries stored of a tensor of `size` > FULL_MAX elements: SUBSET evenly spaced flat indices, first and last included."""
    return np.linspace(0, size - 1, SUBSET).round().astype(np.int64)


def compact(prefix, sd, out):
    """Tensors of at most FULL_MAX elements in full, larger ones as a fixed subset + sum + sum of squares."""
    for k, v in sd.items():
        a = v.detach().double().reshape(-1).numpy()
        if a.size <= FULL_MAX:
            out[f"{prefix}/{k}"] = a.astype(np.float32) if v.dtype != torch.int64 else v.numpy()
        else:
            out[f"{prefix}/{k}@val"] = a[subset_index(a.size)].astype(np.float32)
            out[f"{prefix}/{k}@sum"] = np.array([a.sum(), (a * a).sum()])


def run(mod, init, seqs, items, eps, mirror, dtype):
    torch.manual_seed(1234)
    vae = mod.BCVAE().to(dtype)
    vae.load_state_dict(init)
    vae.train()
    params = list(vae.parameters())
    opt = torch.optim.AdamW(params, lr=LR)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, constant_with_warmup_lambda(0.1 * STEPS))
    shadow = [p.detach().clone() for p in params]
    losses, grads1 = [], None
    for k in range(STEPS):
        x = torch.from_numpy(windows_of(seqs, items[k], mirror)).to(dtype)
        e = torch.from_numpy(eps[k]).to(dtype)
        lat = vae.encode(x)
        z = lat.mean + torch.exp(0.5 * lat.log_var) * e
        y = vae.decode(z)
        reconst, kld, vel = elbo(x, lat.mean, lat.log_var, y)
        loss = reconst + 1.0 * kld + 1.0 * vel
        loss.backward()
        if k == 0:
            grads1 = {n: p.grad.detach().clone() for n, p in vae.named_parameters()}
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        d = ema_decay(k + 1, 0.99)
        with torch.no_grad():
            for s, p in zip(shadow, params):
                s.sub_((1 - d) * (s - p))
        sched.step()
        opt.zero_grad()
        losses.append([float(v.detach()) for v in (reconst, kld, vel, loss)])
    ema = {n: s for (n, _), s in zip(vae.named_parameters(), shadow)}
    return np.array(losses), grads1, vae.state_dict(), ema


def main():
    mod = load_reference_vae()
    lists = reference_lists()
    classes, pairs = lists["default_blendshape_classes"], lists["default_blendshape_classes_mirror_pair"]
    mirror = np.arange(32)
    for l_, r_ in pairs:
        il, ir = classes.index(l_), classes.index(r_)
        mirror[il], mirror[ir] = ir, il
    torch.manual_seed(0)
    init = {k: v.clone() for k, v in mod.BCVAE().state_dict().items()}

    rng = np.random.default_rng(14)
    lengths = np.array([100, 130, 300, 61, 240, 180, 95, 400])
    seqs = []
    for n in lengths:   # smooth coefficient curves in [0, 1]
        t = np.arange(n)[:, None]
        f = rng.uniform(0.01, 0.1, (1, 32))
        ph = rng.uniform(0, 2 * np.pi, (1, 32))
        seqs.append((0.5 + 0.45 * np.sin(f * t + ph) * rng.uniform(0.2, 1.0, (1, 32))).astype(np.float32))
    items = np.zeros((STEPS, BATCH, 4), dtype=np.int32)
    for k in range(STEPS):
        for b in range(BATCH):
            s = int(rng.integers(0, len(seqs)))
            items[k, b] = [s, int(rng.integers(-60, max(0, lengths[s] - 61) + 1)), int(rng.uniform() < 0.5), 0]
    eps = rng.standard_normal((STEPS, BATCH, 64)).astype(np.float32)

    out = {"lengths": lengths, "frames": np.concatenate(seqs, 0), "items": items, "eps": eps, "mirror": mirror.astype(np.int32),
           "classes": np.array(classes), "mirror_pairs": np.array(pairs), "person_ids_train": np.array(lists["person_ids_train"]),
           "person_ids_val": np.array(lists["person_ids_val"]), "lr": np.array(LR)}
    compact("init", init, out)
    l32, _, _, _ = run(mod, init, seqs, items, eps, mirror, torch.float32)
    l64, g64, sd64, ema64 = run(mod, init, seqs, items, eps, mirror, torch.float64)
    out["losses32"], out["losses64"] = l32, l64
    compact("grad1", g64, out)
    compact("final", sd64, out)
    compact("ema", ema64, out)
    path = os.path.join(HERE, "g14_vae_train.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB); fp32 vs fp64 loss max rel {np.abs(l32 / l64 - 1).max():.2e}")


if __name__ == "__main__":
    main()
