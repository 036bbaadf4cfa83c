"""DDPM and DPM-Solver++ host tables (said_amd.scheduler) against the CPU restatement of diffusers 0.19 (tests/sched_ref.py), and the
DDIM tables as they were before the solver column existed.  No GPU."""
import numpy as np
import pytest
import torch

from said_amd import _engine
from said_amd.scheduler import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, SCHEDULERS

import sched_ref

NS = [1, 2, 10, 14, 15, 25, 100, 999]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("N", NS)
def test_dpm_timesteps_match_linspace_restatement(N):
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(N)
    want = sched_ref.dpm_timesteps(N)
    assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), want)
    assert s.num_inference_steps == len(want) == N   # no duplicates below 1000 steps
    assert int(s.timesteps[0]) == 999 and int(s.timesteps[-1]) == round(999 / N)


def test_dpm_timesteps_drop_duplicates_from_1000_steps_on():
    for N in (1000, 1500, 2000):
        s = DPMSolverMultistepScheduler()
        s.set_timesteps(N)
        want = sched_ref.dpm_timesteps(N)
        assert np.array_equal(s.timesteps.numpy(), want) and len(want) < N + 1
        assert len(np.unique(want)) == len(want) == s.num_inference_steps


@pytest.mark.parametrize("N", NS)
def test_ddpm_timesteps_leading(N):
    s = DDPMScheduler()
    s.set_timesteps(N)
    assert np.array_equal(s.timesteps.numpy(), sched_ref.leading_timesteps(N))
    with pytest.raises(ValueError):
        s.set_timesteps(1001)


def _ref_orders(N, start):
    """The order sequence a fresh reference scheduler runs over timesteps[start:] (DPMSolverMultistepScheduler.step's bookkeeping)."""
    r = sched_ref.RefDPM()
    r.set_timesteps(N)
    out, lon = [], 0
    for i in range(start, len(r.timesteps)):
        out.append(r.order_at(i, lon))
        lon = min(lon + 1, 2)
    return out


def test_dpm_order_sequence():
    s = DPMSolverMultistepScheduler()
    for N, want in [(1, [1]), (2, [1, 1]), (3, [1, 2, 1]), (14, [1] + [2] * 12 + [1]), (15, [1] + [2] * 14), (25, [1] + [2] * 24)]:
        s.set_timesteps(N)
        assert s.step_orders() == want == _ref_orders(N, 0), N
    # strength < 1: the loop starts mid-schedule with an empty history (the reference calls set_timesteps fresh)
    for N, start in [(10, 5), (14, 7), (25, 12), (100, 50), (15, 14), (2, 1)]:
        s.set_timesteps(N)
        got = s.step_orders(start)
        assert got == _ref_orders(N, start) and got[0] == 1, (N, start)
        assert got[-1] == (1 if N < 15 else (2 if len(got) > 1 else 1))
        tab = s.coef_table(s.timesteps.numpy()[start:])
        assert list(tab[:, _engine.COEF_SOLVER].astype(int)) == [o + 1 for o in got]


@pytest.mark.parametrize("pred", ["epsilon", "sample", "v_prediction"])
@pytest.mark.parametrize("N", [1, 2, 14, 15, 25, 100])
def test_dpm_coef_table_equals_rowwise_restatement(N, pred):
    s = DPMSolverMultistepScheduler(prediction_type=pred)
    s.set_timesteps(N)
    ts = s.timesteps.numpy()
    r = sched_ref.RefDPM(pred)
    r.set_timesteps(N)
    for start in sorted({0, N // 2, N - 1}):
        sub = ts[start:]
        orders = _ref_orders(N, start)
        want = np.stack([r.row(start + k, orders[k], int(sub[k + 1]) if k + 1 < len(sub) else None) for k in range(len(sub))])
        got = s.coef_table(sub, 0.7)   # (eta is not DPM's: ignored)
        assert got.dtype == np.float32 and got.shape == (len(sub), 8)
        assert np.array_equal(_bits(got), _bits(want)), (N, start)
    assert s.coef_table(ts[:0]).shape == (0, 8)
    with pytest.raises(ValueError):
        s.coef_table(ts[:-1] if N > 1 else np.array([5]))   # not a suffix of the schedule


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("N", [1, 2, 10, 50, 1000])
def test_ddpm_coef_table_equals_rowwise_restatement(N, pred):
    s = DDPMScheduler(prediction_type=pred)
    s.set_timesteps(N)
    ts = s.timesteps.numpy()
    r = sched_ref.RefDDPM(pred)
    r.set_timesteps(N)
    for sub in (ts, ts[N // 3:]):
        want = np.stack([r.row(int(sub[k]), int(sub[k + 1]) if k + 1 < len(sub) else None) for k in range(len(sub))])
        got = s.coef_table(sub, 0.0)
        assert np.array_equal(_bits(got), _bits(want))
        assert np.all(got[:, 7] == 1.0)
    assert s.coef_table(ts, 0.0)[-1, 4] == 0.0 and int(ts[-1]) == 0   # no noise on the step to t = 0
    assert np.all(s.coef_table(ts, 0.0)[:-1, 4] > 0)


def _ddim_table_before_solver_column(s, timesteps, eta):
    """DDIMScheduler.coef_table as it stood before column 7 carried a solver code (column 7 was always 0 then)."""
    n = len(timesteps)
    if n == 0:
        return np.zeros((0, 8), np.float32)
    ts = torch.as_tensor(np.asarray(timesteps, dtype=np.int64))
    ac = s.alphas_cumprod
    prev = ts - s.config.num_train_timesteps // s.num_inference_steps
    a_t = ac[ts]
    a_p = torch.where(prev >= 0, ac[prev.clamp(min=0)], s.final_alpha_cumprod.to(ac.dtype))
    b_t = 1 - a_t
    b_p = 1 - a_p
    variance = (b_p / b_t) * (1 - a_t / a_p)
    std_dev_t = eta * variance ** (0.5)
    tab = torch.zeros(n, 8, dtype=torch.float32)
    tab[:, 0] = a_t ** (0.5)
    tab[:, 1] = b_t ** (0.5)
    tab[:, 2] = a_p ** (0.5)
    tab[:, 3] = (1 - a_p - std_dev_t ** 2) ** (0.5)
    tab[:, 4] = std_dev_t
    tab[:, 5], tab[:, 6] = 1.0, 0.0
    if n > 1:
        a_n = ac[ts[1:]]
        tab[:-1, 5] = a_n ** 0.5
        tab[:-1, 6] = (1 - a_n) ** 0.5
    return tab.numpy()


@pytest.mark.parametrize("N,eta,start", [(50, 0.0, 0), (25, 1.0, 0), (1000, 0.3, 0), (30, 0.0, 12), (7, 0.5, 3), (1, 0.0, 0)])
def test_ddim_tables_unchanged_with_solver_column_zero(N, eta, start):
    s = DDIMScheduler()
    s.set_timesteps(N)
    ts = s.timesteps.numpy()[start:]
    got = s.coef_table(ts, eta)
    assert np.all(got[:, _engine.COEF_SOLVER] == 0.0)
    assert got.tobytes() == _ddim_table_before_solver_column(s, ts, eta).tobytes()
    assert s.draws_step_noise(eta) == (eta > 0)


def test_scheduler_protocol_and_defaults():
    assert set(SCHEDULERS) == {"ddim", "ddpm", "dpmsolver++"}
    for cls in (DDPMScheduler, DPMSolverMultistepScheduler):
        s = cls(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", prediction_type="v_prediction")   # SAID.__init__'s call
        for attr in ("config", "timesteps", "alphas_cumprod", "init_noise_sigma", "set_timesteps", "scale_model_input", "add_noise",
                     "get_velocity", "coef_table", "step"):
            assert hasattr(s, attr), (cls.__name__, attr)
        assert s.init_noise_sigma == 1.0 and s.config.prediction_type == "v_prediction"
        x = torch.randn(2, 3)
        assert s.scale_model_input(x, 5) is x
        assert torch.equal(s.alphas_cumprod, DDIMScheduler().alphas_cumprod)
        with pytest.raises(NotImplementedError):
            cls(beta_schedule="linear")
    assert DDPMScheduler().draws_step_noise(0.0) and not DPMSolverMultistepScheduler().draws_step_noise(1.0)
    c = DDPMScheduler().config
    assert (c.variance_type, c.clip_sample, c.clip_sample_range, c.timestep_spacing, c.steps_offset) == ("fixed_small", True, 1.0, "leading", 0)
    c = DPMSolverMultistepScheduler().config
    assert (c.algorithm_type, c.solver_order, c.solver_type, c.lower_order_final, c.thresholding, c.use_karras_sigmas) == \
        ("dpmsolver++", 2, "midpoint", True, False, False)


def test_dpm_lambda_table_is_the_constructors():
    s, r = DPMSolverMultistepScheduler(), sched_ref.RefDPM()
    for a, b in ((s.alpha_t, r.alpha_t), (s.sigma_t, r.sigma_t), (s.lambda_t, r.lambda_t)):
        assert torch.equal(a, b)


class _ForeignScheduler:   # e.g. a diffusers instance: the generic protocol, not the engine's tables
    config = None
    timesteps = torch.arange(10)
    init_noise_sigma = 1.0

    def set_timesteps(self, n, device=None):
        pass

    def step(self, *a, **k):
        raise AssertionError("never reached")


def test_foreign_scheduler_is_refused_before_gpu_work():
    from said_amd.model.diffusion import SAID_UNet1D
    m = SAID_UNet1D()
    m.noise_scheduler = _ForeignScheduler()
    with pytest.raises(TypeError, match="DPMSolverMultistepScheduler"):
        m.inference(torch.zeros(1, 1600), num_inference_steps=5)
    assert m._eng is None


def test_dpm_out_of_range_indexing_raises_like_the_reference():
    """From 1000 steps on DPM-Solver++ has fewer timesteps than num_inference_steps: where the reference's timesteps[-init_timestep]
    (diffusion.py:375) or timesteps[tdx_next] (:451) would raise IndexError, SAID.inference raises ValueError before any GPU work."""
    from said_amd.model.diffusion import SAID_UNet1D
    m = SAID_UNet1D()
    m.noise_scheduler = DPMSolverMultistepScheduler()
    init = torch.rand(1, 6, 32)
    with pytest.raises(ValueError, match="strength"):
        m.inference(torch.zeros(1, 1600), init_samples=init, num_inference_steps=2000, strength=1.0)
    with pytest.raises(ValueError, match="masked editing"):
        m.inference(torch.zeros(1, 1600), init_samples=init, mask=torch.ones_like(init), num_inference_steps=1500, strength=0.5)
    assert m._eng is None
    with pytest.raises(_engine.EngineError):   # 1500 steps from strength 0.25 run on (the reference would not raise either): the CPU model is refused
        m.inference(torch.zeros(1, 1600), init_samples=init, mask=torch.ones_like(init), num_inference_steps=1500, strength=0.25)
