"""What the CPU and the GPU tests of the Q-network's training-mode dropout share (tests/test_qnet_dropout_host.py,
tests/test_gpu_qnet_dropout.py).

The mask rule, restated in NumPy uint32 from its specification (include/g2048_train.h), not imported from the library: for the
library call with index c, (k0, k1) = rng_keys(seed, 12, c); element e of site s of encoder layer L draws
h = rng_draw(k0, k1, ((4 L + s) << 32) | e, 0) and is kept iff h >= T = floor(p_s 2^32); a kept element is multiplied by
1 / (1 - p_s), a dropped one by 0. Site 0: the attention probabilities, e = (head n + query) n + key, matrix (8 n, n); sites 1 and 3:
dropout1 / dropout2, e = row 128 + feature, (n, 128); site 2: the hidden layer's dropout, e = row dim_ff + feature, (n, dim_ff). The
hash itself (splitmix64, rng_keys, rng_draw) is the restatement tests/ppo_dropout_ref.py already holds.

The yardstick: the STOCK module in .train() mode, fed those masks by replacing torch.nn.functional.dropout and
torch.nn.functional.scaled_dot_product_attention for the duration of a call (feeding()). The training-mode layer calls them in the
order SDPA (1, 8, n, 16), dropout (n, 1, 128), (n, 1, dim_ff), (n, 1, 128) per layer, which is the order of the sites; every call
asserts its shape and the probability torch passes. qnet_grad_ref.stock_loss_grad on such a module in float64 (scale 1 / (1 - p) in
double) is the reference, the same module in float32 (the float scale) the tolerance's measure: per tensor
max|got - f64| / max|f64| <= 8 x the float32 run's worst such ratio over the gradient tensors of the same case (the rule of
tests/test_gpu_qnet_grad.py), and that ratio itself must lie in (0, FAIR_F32] (tests/test_qnet_dropout_host.py asserts it for every
case below, on the CPU). DROPOUT_SEED is the first seed from 0 upwards for which that holds in every case; the host test checks it.
"""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

import encoder_dropout_ref as E
import qnet_grad_ref as R
from ppo_dropout_ref import scale32  # noqa: F401  (tests/test_qnet_dropout_host.py reads it from here)

DOMAIN = 12
DROPOUT_SEED = 0                      # the online network's; the target network's is DROPOUT_SEED + 1
HIGH_INDEX = (1 << 32) + 7            # a call index above 2^32
FAIR_F32 = 1e-5                       # tests/test_gpu_qnet_batch.py's: above this stock float32 is no yardstick
P4 = (0.1, 0.1, 0.1, 0.1)
UNEQUAL = (0.3, 0.0, 0.2, 0.1)        # a site with p = 0 next to live ones, no two sites alike
SIZES = (1, 2, 15, 16, 17, 33, 257)   # every tile edge of the touched kernels
EARLY_SHAPES = ((2, 64, 2), (12, 32, 1))          # (model seed, dim_ff, layers), tests/test_gpu_qnet_grad.py's SHAPES
REGIME_SHAPES = (("mid", 64, 2), ("distinct", 160, 3))
# (kind, shape, n, p4, call index): the loss-and-gradient cases of the GPU test
LOSS_CASES = ([("early", s, n, P4, 7) for s in EARLY_SHAPES for n in SIZES]
              + [("regime", s, n, P4, 7) for s in REGIME_SHAPES for n in (17, 257)]
              + [("early", EARLY_SHAPES[0], 17, (0.5,) * 4, 7), ("early", EARLY_SHAPES[0], 17, UNEQUAL, HIGH_INDEX)])
FORWARD_SIZES = (17, 257)             # forward_batch(training=True) and dqn_targets(training=True), on EARLY_SHAPES[0]
# the closed round; lr is the floor of the reference's cosine schedule (g2048.cosine_lr's eta_min): AdamW's first steps move every
# weight by about lr whatever its gradient's size, so at 1e-3 the float32 module's second step sits at 8.9e-6 of the fairness bound
ROUND_N, ROUND_STEPS, ROUND_LR, GAMMA = 48, 2, 1e-4, 0.99


def case_id(case):
    kind, shape, n, p4, index = case
    return "%s-%s-n%d-p%s%s" % (kind, "-".join(map(str, shape)), n, "_".join("%g" % p for p in sorted(set(p4), reverse=True)) if len(set(p4)) > 1
                                else "%g" % p4[0], "-hi" if index >= 1 << 32 else "")


# ------------------------------------------------------------------------------------------------------ the mask rule --
def site_shape(site, n, dim_ff):
    return (8 * n, n) if site == 0 else (n, dim_ff if site == 2 else 128)


ENCODER = E.Encoder(DOMAIN, site_shape, lambda n: (1, 8, n, 16), lambda n, width: (n, 1, width), lambda model: model.transformer.layers)
# the mask rule and the stock module, masked (encoder_dropout_ref.py)
keep_mask, multiplier, feeding, training_copy, dims = (ENCODER.keep_mask, ENCODER.multiplier, ENCODER.feeding, ENCODER.training_copy,
                                                       ENCODER.dims)


def masked_loss_grad(model, p4, seed, call_index, codes, actions, targets, weights):
    """qnet_grad_ref.stock_loss_grad of the training-mode module (training_copy) under the masks of (seed, call_index)."""
    dim_ff, layers = dims(model)
    with feeding(seed, call_index, p4, len(codes), dim_ff) as calls:
        out = R.stock_loss_grad(model, codes, actions, targets, weights)
    assert calls[0] == 4 * layers
    return out


@torch.no_grad()
def masked_forward(model, p4, seed, call_index, codes):
    """q (n, 4) float64 NumPy of the training-mode module's batch call under the masks of (seed, call_index)."""
    dim_ff, layers = dims(model)
    dtype = next(model.parameters()).dtype
    with feeding(seed, call_index, p4, len(codes), dim_ff) as calls:
        q = model(R.tile_values(codes, dtype))
    assert calls[0] == 4 * layers
    return q.numpy().astype(np.float64)


@torch.no_grad()
def plain_forward(model, p4, seed, call_index, codes):
    """The same function with plain torch ops in the module's dtype, no module called: conv, embedding, per layer in_proj, 8 heads
    of 16, softmax(q k^T / 4) x m0, . v, x + out_proj(..) x m1, norm1, relu(linear1) x m2, x + linear2(..) x m3, norm2; fc."""
    n, dtype = len(codes), next(model.parameters()).dtype
    dim_ff, _ = dims(model)
    m = lambda layer, site: multiplier(seed, call_index, layer, site, p4[site], n, dim_ff, dtype)
    x = model.embedding(model.cnn(R.tile_values(codes, dtype).view(-1, 1, 4, 4)).view(n, -1))
    for L, lay in enumerate(model.transformer.layers):
        a = lay.self_attn
        q, k, v = (x @ a.in_proj_weight.T + a.in_proj_bias).split(128, dim=1)
        q, k, v = (t.reshape(n, 8, 16).transpose(0, 1) for t in (q, k, v))
        prob = torch.softmax(q @ k.transpose(1, 2) / 4.0, dim=-1) * m(L, 0).reshape(8, n, n)
        att = (prob @ v).transpose(0, 1).reshape(n, 128)
        x = F.layer_norm(x + (att @ a.out_proj.weight.T + a.out_proj.bias) * m(L, 1), (128,), lay.norm1.weight, lay.norm1.bias, lay.norm1.eps)
        h = torch.relu(x @ lay.linear1.weight.T + lay.linear1.bias) * m(L, 2)
        x = F.layer_norm(x + (h @ lay.linear2.weight.T + lay.linear2.bias) * m(L, 3), (128,), lay.norm2.weight, lay.norm2.bias, lay.norm2.eps)
    return (x @ model.fc.weight.T + model.fc.bias).numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ the cases --
@functools.lru_cache(maxsize=None)
def case_model(kind, shape):
    """(the eval-mode float32 module on the CPU, the boards of its largest size) of a case."""
    from test_gpu_qnet_batch import RAGGED, regime_boards, regime_model
    from test_policy_host import random_boards
    from test_qnet_host import random_model
    if kind == "early":                # tests/test_gpu_qnet_grad.py random_case's module and boards
        seed, dim_ff, layers = shape
        return random_model(seed, dim_ff, layers), (random_boards(max(RAGGED), 9 + seed) % 4).astype(np.uint8)
    return regime_model(*shape), regime_boards(shape[0], 257)


@functools.lru_cache(maxsize=None)
def loss_case(case, seed=DROPOUT_SEED):
    """(model, boards, actions, targets, weights, float64 (loss, td, q, grads), float32 the same) of a loss-and-gradient case: the
    inputs by qnet_grad_ref's recipe around the eval-mode float64 module's own Q, the references the masked training-mode modules'
    (shared, never modified)."""
    kind, shape, n, p4, index = case
    model, boards = case_model(kind, shape)
    boards = boards[:n]
    a, t, w = R.case_inputs(copy.deepcopy(model).double(), boards)
    want, f32 = (masked_loss_grad(training_copy(model, p4, dtype), p4, seed, index, boards, a, t, w) for dtype in (torch.float64, torch.float32))
    return model, boards, a, t, w, want, f32


def yardstick(want, f32):
    """The float32 masked module's worst gradient tensor against the float64 one's: the measure the bound is 8 x of."""
    return R.ratios(f32[3], want[3]).max()


@functools.lru_cache(maxsize=None)
def forward_case(n, seed=DROPOUT_SEED):
    """Test 4's references at n boards on EARLY_SHAPES[0]: the online network (seed, call index 3) and a target network (weights
    of model seed + 1, dropout seed + 1, call index 5) on the same next boards; shaped rewards and dones by a recipe. Returns
    (online model, target model, boards, shaped, dones, per dtype (q_online, q_target)) with dtype float64 first."""
    from test_qnet_host import random_model
    mseed, dim_ff, layers = EARLY_SHAPES[0]
    online, boards = case_model("early", EARLY_SHAPES[0])
    target = random_model(mseed + 1, dim_ff, layers)
    boards = boards[:n]
    i = np.arange(n)
    shaped, dones = (((7 * i) % 13 - 6) / 4.0).astype(np.float32), (i % 5 == 0).astype(np.float32)
    qs = [(masked_forward(training_copy(online, P4, dt), P4, seed, 3, boards), masked_forward(training_copy(target, P4, dt), P4, seed + 1, 5, boards))
          for dt in (torch.float64, torch.float32)]
    return online, target, boards, shaped, dones, qs


def dqn_targets_of(q_online, q_target, shaped, dones, gamma=GAMMA):
    """(targets, next actions, the online Q's margin between its two best actions per row) in float64."""
    a = q_online.argmax(1)
    top = np.sort(q_online, axis=1)
    return shaped + (1.0 - dones) * gamma * q_target[np.arange(len(a)), a], a, top[:, -1] - top[:, -2]


# ------------------------------------------------------------------------------------------------------ one closed round --
def flat_of(model, dtype=None):
    """The module's parameters as one flat tensor in the plain layout's order (the module's parameter order), without the eps slots."""
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).to(dtype or next(model.parameters()).dtype)


@torch.no_grad()
def load_flat(model, flat):
    o = 0
    for p in model.parameters():
        p.copy_(flat[o:o + p.numel()].view(p.shape))
        o += p.numel()


@functools.lru_cache(maxsize=None)
def closed_round(dtype, seed=DROPOUT_SEED):
    """ROUND_STEPS train steps at ROUND_N boards on the masked stock modules in dtype: per step dqn_targets with both networks in
    training mode (the online network's call index, then the target's), the loss and gradients on the online network (its next
    index), clipping and AdamW by g2048.qnet.adamw_step_reference. The online network's dropout seed is `seed`, the target's
    seed + 1; both count their indices from 0. Returns (inputs, per step a dict of float64 NumPy: targets, next_actions, margin,
    loss, td, q, grads, params after the step)."""
    from g2048 import qnet
    from test_qnet_host import random_model
    mseed, dim_ff, layers = EARLY_SHAPES[0]
    base, boards = case_model("early", EARLY_SHAPES[0])
    n = ROUND_N
    boards, next_boards = boards[:n], boards[n:2 * n]
    online, target = training_copy(base, P4, dtype), training_copy(random_model(mseed + 1, dim_ff, layers), P4, dtype)
    i = np.arange(n)
    actions, _, weights = R.recipe(n)
    shaped, dones = (((7 * i) % 13 - 6) / 4.0).astype(np.float32), (i % 5 == 0).astype(np.float32)
    idx_online = idx_target = 0
    m = v = torch.zeros_like(flat_of(online))
    steps = []
    for step in range(1, ROUND_STEPS + 1):
        q_on = masked_forward(online, P4, seed, idx_online, next_boards)
        q_t = masked_forward(target, P4, seed + 1, idx_target, next_boards)
        idx_online, idx_target = idx_online + 1, idx_target + 1
        targets, next_a, margin = dqn_targets_of(q_on, q_t, shaped, dones)
        targets = targets.astype(np.float32)
        loss, td, q, grads = masked_loss_grad(online, P4, seed, idx_online, boards, actions, targets, weights)
        idx_online += 1
        g = torch.from_numpy(np.concatenate(grads)).to(dtype)
        p, _, m, v, norm = qnet.adamw_step_reference(flat_of(online), g, m, v, [], ROUND_LR, step, dtype=dtype)
        load_flat(online, p)
        steps.append(dict(targets=targets.astype(np.float64), next_actions=next_a, margin=margin, loss=loss, td=td, q=q, grads=grads,
                          params=p.numpy().astype(np.float64), norm=float(norm)))
    return (boards, next_boards, actions, weights, shaped, dones), steps
