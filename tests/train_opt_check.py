"""One clip + AdamW + EMA update of a trainer (said_amd/csrc/train_opt.hip) from set gradients, against torch's fp32 clip_grad_norm_ and AdamW
and the EMA formula.  Both trainers run the same kernels: tests/test_gpu_vae_train.py and tests/test_gpu_unet_train.py call this with their own
trainer."""
import numpy as np
import torch

from said_amd.util.scheduler import ema_decay


def ulp_distance(a, b, mag, ulps):
    """(ok, the worst |a - b| in units in the last place); ok: every |a - b| is within `ulps` of them.  The unit is that of the largest
    magnitude among a, b and the update's operands (`mag`): a result that cancels (an EMA shadow or a parameter landing near 0) carries the
    rounding of its operands, not of itself."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    sp = np.spacing(np.maximum(np.maximum(np.abs(a), np.abs(b)), np.abs(np.asarray(mag, np.float32))))
    tol = ulps * sp + 1e-30
    d = np.abs(a.astype(np.float64) - b)
    return bool(np.all(d <= tol)), float((d / sp).max())


def check_clip_adamw_ema_update(tr, copies, scalars, grad_scale, grad_div, bounds=(4, 4, 4, 8)):
    """`copies`: the trainer's (STATE, GRAD, EXP_AVG, EXP_AVG_SQ, EMA) selectors; `scalars(k)`: its step record of optimizer step k; the drawn
    gradients are scaled by grad_scale / grad_div, with grad_div near sqrt(number of parameters) so that the norm is near grad_scale;
    `bounds`: the distance in ulps (ulp_distance) allowed to the parameters, exp_avg, exp_avg_sq and the EMA shadow."""
    state, grad, exp_avg, exp_avg_sq, ema = copies
    rng = np.random.default_rng(int(grad_scale * 1000))
    k = 6   # optimizer step 7: past the warmup, bias corrections still active
    names = list(tr.parameters_of(state).keys())
    shapes = {n: t.shape for n, t in tr.parameters_of(state).items()}
    vals = {}
    for n in names:
        p, g, m = (rng.standard_normal(shapes[n]).astype(np.float32) for _ in range(3))
        v, e = rng.random(shapes[n]).astype(np.float32) * 1e-3, rng.standard_normal(shapes[n]).astype(np.float32)
        g *= grad_scale / grad_div
        vals[n] = (p, g, m, v, e)
        for which, a in zip((state, grad, exp_avg, exp_avg_sq, ema), (p, g, m, v, e)):
            tr.eng.set_tensor(which, n, a)
    tr.eng.apply_update(scalars(k))
    # torch, fp32
    params = [torch.tensor(vals[n][0], requires_grad=True) for n in names]
    for q, n in zip(params, names):
        q.grad = torch.tensor(vals[n][1])
    norm = torch.nn.utils.clip_grad_norm_(params, 1.0)
    assert (norm.item() > 1.0) == (grad_scale > 1)
    lr = tr.lr_at(k)
    opt = torch.optim.AdamW(params, lr=lr)
    for q, n in zip(params, names):
        opt.state[q] = {"step": torch.tensor(float(k)), "exp_avg": torch.tensor(vals[n][2]), "exp_avg_sq": torch.tensor(vals[n][3])}
    opt.step()
    d = ema_decay(k + 1, tr.ema_decay)
    worst, bad = np.zeros(4), []
    for q, n in zip(params, names):
        e = torch.tensor(vals[n][4])
        e.sub_((1 - d) * (e - q.detach()))
        p0, g0, m0, v0, e0 = vals[n]
        res = [ulp_distance(tr._get(state, n).numpy(), q.detach().numpy(), p0, bounds[0]),
               ulp_distance(tr._get(exp_avg, n).numpy(), opt.state[q]["exp_avg"].numpy(), np.maximum(np.abs(m0), np.abs(g0)), bounds[1]),
               ulp_distance(tr._get(exp_avg_sq, n).numpy(), opt.state[q]["exp_avg_sq"].numpy(), np.maximum(v0, g0 * g0), bounds[2]),
               ulp_distance(tr._get(ema, n).numpy(), e.numpy(), np.maximum(np.abs(e0), np.abs(p0)), bounds[3])]
        worst = np.maximum(worst, [u for _, u in res])
        bad += [(n, c, u) for c, (ok, u) in zip(("state", "exp_avg", "exp_avg_sq", "ema"), res) if not ok]
    print(f"clip + AdamW + EMA, grad_scale {grad_scale}: norm {norm.item():.6g}, worst distance in ulps: state {worst[0]:.3g}, "
          f"exp_avg {worst[1]:.3g}, exp_avg_sq {worst[2]:.3g}, ema {worst[3]:.3g}")
    assert not bad, bad[:8]
