"""What the CPU and the GPU tests of the PPO update's device step (g2048_ppo_adam_step, DevicePPOLearner.adam_step / update) share:
the yardstick, the two networks' start weights and the seeded gradients of the four-step case, and the measures of the tolerance.

The yardstick is adam_step_reference below: clip_grad_norm_(max_norm) followed by Adam.step() number `step` on ONE network's flat
buffers, built as g2048.qnet.adamw_step_reference is (norm summed in float64, the scalars formed in Python floats as torch's Adam
forms them) without weight decay and without LayerNorm-eps slots. tests/test_ppo_step_host.py holds it to stock clip_grad_norm_ +
torch.optim.Adam on the reference-layout modules in float64. The tolerance's measure is this function run in float32.

Tolerance (tests/test_gpu_qnet_step.py's): per buffer max|device - y64| / max|y64| <= F32_FACTOR x the same measure of the float32
yardstick, both fed the device's own pre-step state."""
import functools

import numpy as np
import torch

import ppo_update_ref as R
from ppo_update_ref import F32_FACTOR  # noqa: F401  (re-exported)

ACTOR_FLOATS, CRITIC_FLOATS = 46532, 46337
FLOATS = (ACTOR_FLOATS, CRITIC_FLOATS)
MAX_NORM = R.MAX_NORM                                    # 0.5, PPOAgent's own
LR = (R.LR_ACTOR, R.LR_CRITIC)                           # 8e-4, 2e-3
EPS = (1e-8, 3e-8)                                       # differ per network, as the learning rates do
BETAS = (0.9, 0.999)
# the gradient norm as a multiple of MAX_NORM, step by step
ACTOR_FACTORS, CRITIC_FACTORS = (2.0, 1.0, 0.5, 0.5), (0.5, 2.0, 1.0, 0.5)
FACTORS = (ACTOR_FACTORS, CRITIC_FACTORS)
GRAD_SEED = 250


@torch.no_grad()
def adam_step_reference(plain, grad, exp_avg, exp_avg_sq, lr, step, betas=BETAS, eps=1e-8, max_norm=MAX_NORM, dtype=torch.float64):
    """clip_grad_norm_(max_norm) followed by Adam.step() number `step` (>= 1) on one network's flat buffers, with plain torch ops in
    `dtype`. With norm = ||grad|| (summed in float64, then rounded to `dtype`) and c = min(1, max_norm / (norm + 1e-6)) (max_norm
    None: no clipping),
        g = grad c;  m = m + (g - m)(1 - beta1);  v = v beta2 + (g g)(1 - beta2);
        p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps)),  bc1 = 1 - beta1^step, bc2 = 1 - beta2^step.
    A norm that is not finite changes nothing. Returns new (plain, grad, exp_avg, exp_avg_sq, norm) in `dtype`."""
    p0, g0, m0, v0 = (torch.as_tensor(t).detach().to(dtype) for t in (plain, grad, exp_avg, exp_avg_sq))
    norm = torch.linalg.vector_norm(g0, dtype=torch.float64).to(dtype)
    if not bool(torch.isfinite(norm)):
        return p0.clone(), g0.clone(), m0.clone(), v0.clone(), norm
    beta1, beta2 = betas
    c = torch.clamp((norm + 1e-6).reciprocal() * (float("inf") if max_norm is None else max_norm), max=1.0)      # torch's max_norm / tensor
    g = g0 * c
    m = m0 + (g - m0) * (1 - beta1)
    v = v0 * beta2 + (g * g) * (1 - beta2)
    p = p0 - (lr / (1 - beta1 ** step)) * (m / (v.sqrt() / (1 - beta2 ** step) ** 0.5 + eps))
    return p, g, m, v, norm


def yardsticks(pre, which, step, lr=LR, eps=EPS, max_norm=MAX_NORM):
    """(float64 yardstick, float32 yardstick) of network `which` (0 actor, 1 critic) from its pre-step (plain, grad, exp_avg,
    exp_avg_sq): each the new (plain, grad, exp_avg, exp_avg_sq) as float64 NumPy."""
    return tuple(tuple(t.numpy().astype(np.float64) for t in adam_step_reference(*pre, lr[which], step, eps=eps[which], max_norm=max_norm,
                                                                                 dtype=dtype)[:4])
                 for dtype in (torch.float64, torch.float32))


def deviation(got, y64):
    """max|got - y64| / max|y64| of one buffer."""
    return float(np.abs(np.asarray(got, np.float64) - y64).max() / np.abs(y64).max())


def flat_of(module):
    """The module's parameters in the plain layout (named_parameters() order), float32."""
    return torch.cat([p.detach().reshape(-1) for p in module.parameters()]).float().contiguous()


def spread_gradient(rng, floats, norm):
    """A seeded gradient of `floats` float32 with magnitudes over several decades and the given norm."""
    g = rng.normal(0.0, 1.0, floats) * np.exp(rng.normal(0.0, 2.0, floats))
    return torch.from_numpy((g * (norm / np.linalg.norm(g))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def step_case():
    """((actor plain, critic plain), grads[step][network]) of the four-step case: R.make_modules()'s weights in the plain layout and
    seeded gradients whose norms are FACTORS x MAX_NORM (shared, never modified)."""
    nets = R.make_modules()
    plains = tuple(flat_of(net) for net in nets)
    assert tuple(p.numel() for p in plains) == FLOATS
    rng = np.random.default_rng(GRAD_SEED)
    grads = [tuple(spread_gradient(rng, FLOATS[k], FACTORS[k][s] * MAX_NORM) for k in (0, 1)) for s in range(4)]
    return plains, grads


def clip_coefficient(norm, max_norm=MAX_NORM):
    """c in float64 from a norm given as a float32 value."""
    return min(1.0, max_norm / (np.float64(np.float32(norm)) + 1e-6))


def run_reference(steps, step_numbers, dtype=torch.float64):
    """The case's networks through the given steps' gradients with the given Adam step numbers, from zero moments: per network the
    final (plain, grad, exp_avg, exp_avg_sq) as float64 NumPy."""
    plains, grads = step_case()
    out = []
    for k in (0, 1):
        state = (plains[k], None, torch.zeros(FLOATS[k]), torch.zeros(FLOATS[k]))
        for s, number in zip(steps, step_numbers):
            p, g, m, v, _ = adam_step_reference(state[0], grads[s][k], state[2], state[3], LR[k], number, eps=EPS[k], dtype=dtype)
            state = (p, g, m, v)
        out.append(tuple(t.numpy().astype(np.float64) for t in state))
    return out
