"""What the CPU and the GPU tests of the transformer policy's device step (g2048_tpolicy_adam_step, DeviceTransformerPolicy.adam_step /
update) share: the yardstick, the start weights and seeded gradients of the four-step case, and the measures of the tolerance.

The yardstick is ppo_step_ref.adam_step_reference (clip_grad_norm_(max_norm) followed by Adam.step() number `step` on one flat
buffer, the norm summed in float64, the scalars formed in Python floats as torch's Adam forms them) plus a mask: the two
LayerNorm-eps slots of every layer are settings and keep their bits in all four buffers. tests/test_tpolicy_step_host.py holds it
to stock clip_grad_norm_ + torch.optim.Adam on the float64 module. The tolerance's measure is this function run in float32.

Tolerance (tests/test_gpu_ppo_step.py's): per buffer max|device - y64| / max|y64| <= F32_FACTOR x the same measure of the float32
yardstick, both fed the device's own pre-step state.

The case's weights: the hash-derived weights of tests/golden/tpolicy.npz (test_tpolicy_host.golden_model) at the reference's shape,
tpolicy_grad_ref.stock_module's at every other. The gradients are ppo_step_ref.spread_gradient ones with their eps slots set to 0
(as g2048_tpolicy_loss_grad leaves them), scaled to norms of FACTORS x MAX_NORM: clipped, at the edge, unclipped twice."""
import functools

import numpy as np
import torch

import ppo_step_ref as S
import tpolicy_grad_ref as G
from ppo_step_ref import F32_FACTOR, clip_coefficient, deviation  # noqa: F401  (re-exported)
from test_tpolicy_host import golden_model

MAX_NORM = S.MAX_NORM                                    # 0.5, PPOAgent's own
LR = 3e-4                                                # examples/tpolicy_update.py's default: the reference never trains this model
EPS = 1e-8
BETAS = S.BETAS
FACTORS = (2.0, 1.0, 0.5, 0.5)                           # the gradient norm as a multiple of MAX_NORM, step by step
GRAD_SEED = 300
# (dim_ff, layers): a tail group of 3 floats and the eps pair in one half of a group; a tail of 1 float and the pairs in both halves;
# the reference's shape; a shape at which the chunk rule gives a norm block two passes of its threads
SHAPES = ((32, 1), (96, 2), (2048, 2), (4096, 2))


def plain_floats(dim_ff, layers):
    return 128 + layers * (16962 + 129 * dim_ff) + 139781


def eps_slots(dim_ff, layers):
    """The flat indices of the LayerNorm-eps slots: the last two floats of every layer's block; blocks start at float 128."""
    length = 16962 + 129 * dim_ff
    return np.array([128 + (l + 1) * length - 2 + j for l in range(layers) for j in (0, 1)], dtype=np.int64)


@torch.no_grad()
def adam_step_reference(plain, grad, exp_avg, exp_avg_sq, eps_at, lr, step, betas=BETAS, eps=EPS, max_norm=MAX_NORM, dtype=torch.float64):
    """ppo_step_ref.adam_step_reference over the whole buffer (the norm too), then the slots eps_at of all four buffers put back to
    what they were. Returns new (plain, grad, exp_avg, exp_avg_sq, norm) in `dtype`; the arguments are not modified."""
    before = [torch.as_tensor(t).detach().to(dtype) for t in (plain, grad, exp_avg, exp_avg_sq)]
    p, g, m, v, norm = S.adam_step_reference(plain, grad, exp_avg, exp_avg_sq, lr, step, betas=betas, eps=eps, max_norm=max_norm, dtype=dtype)
    at = torch.as_tensor(eps_at, dtype=torch.int64)
    for new, old in zip((p, g, m, v), before):
        new[at] = old[at]
    return p, g, m, v, norm


def yardsticks(pre, eps_at, step, lr=LR, eps=EPS, max_norm=MAX_NORM):
    """(float64 yardstick, float32 yardstick) from the pre-step (plain, grad, exp_avg, exp_avg_sq): each the new four buffers as
    float64 NumPy."""
    return tuple(tuple(t.numpy().astype(np.float64) for t in adam_step_reference(*pre, eps_at, lr, step, eps=eps, max_norm=max_norm,
                                                                                 dtype=dtype)[:4])
                 for dtype in (torch.float64, torch.float32))


@functools.lru_cache(maxsize=None)
def module_of(dim_ff, layers):
    """The case's float32 module in eval mode (shared, never modified)."""
    if (dim_ff, layers) == (2048, 2):
        return golden_model()[1].float().eval()
    return G.stock_module(dim_ff, layers)


def flat_of(module, dtype=torch.float32):
    """The module's plain buffer (g2048.tpolicy.flatten's, the eps slots holding the LayerNorms' eps), in dtype."""
    from g2048 import tpolicy
    return tpolicy.flatten(tpolicy.parse(module)).to(dtype).contiguous()


def spread_gradient(rng, dim_ff, layers, norm):
    """ppo_step_ref.spread_gradient with the eps slots 0 and the norm restored."""
    g = S.spread_gradient(rng, plain_floats(dim_ff, layers), 1.0).numpy().astype(np.float64)
    g[eps_slots(dim_ff, layers)] = 0.0
    return torch.from_numpy((g * (norm / np.linalg.norm(g))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def step_case(dim_ff, layers):
    """(plain float32, [the four steps' gradients]) of a shape (shared, never modified)."""
    plain = flat_of(module_of(dim_ff, layers))
    assert plain.numel() == plain_floats(dim_ff, layers)
    rng = np.random.default_rng(GRAD_SEED + dim_ff + layers)
    return plain, [spread_gradient(rng, dim_ff, layers, f * MAX_NORM) for f in FACTORS]


def run_reference(dim_ff, layers, steps, step_numbers, dtype=torch.float64):
    """The case through the given steps' gradients with the given Adam step numbers, from zero moments: the final (plain, grad,
    exp_avg, exp_avg_sq) as float64 NumPy."""
    plain, grads = step_case(dim_ff, layers)
    at, n = eps_slots(dim_ff, layers), plain.numel()
    state = (plain, None, torch.zeros(n), torch.zeros(n))
    for s, number in zip(steps, step_numbers):
        state = adam_step_reference(state[0], grads[s], state[2], state[3], at, LR, number, dtype=dtype)[:4]
    return tuple(t.numpy().astype(np.float64) for t in state)


# The clip coefficient's two float32 forms, (1 / (norm + 1e-6)) max_norm (torch's, the kernel's) and max_norm / (norm + 1e-6), are the
# same bits whenever max_norm is a power of two, PPOAgent's 0.5 included. At max_norm 0.3 they differ at these multiples of the second
# step's gradient (norms 0.685 and 2.95): the one case in which a clipped gradient tells them apart.
CLIP_FORM_MAX_NORM, CLIP_FORM_SCALES = 0.3, (1.37, 5.9)


def clip_forms(norm, max_norm):
    """(reciprocal first, direct quotient) in float32 arithmetic from a float32 norm, each operation rounded on its own."""
    f = np.float32
    d = f(f(norm) + f(1e-6))
    return min(f(1.0), f(f(f(1.0) / d) * f(max_norm))), min(f(1.0), f(f(max_norm) / d))
