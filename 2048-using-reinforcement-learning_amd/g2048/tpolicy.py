"""The reference's transformer policy (models/transformer.py:4-40) as one HIP launch on the packed boards, and its PPO update on
the device.

`DeviceTransformerPolicy(model, precision="f32")` takes a torch module of that structure, flattens its parameters into the
plain layout of include/g2048.h (state-dict order, plus the two LayerNorm eps per layer), packs them with `g2048_tpolicy_pack`
and runs `g2048_tpolicy_forward` on uint8 (N,16) boards.

The module is recognised by structure, not by attribute names: exactly one nn.TransformerEncoder (post-norm ReLU layers,
d_model 64, 4 heads, batch_first, no final norm, dim_feedforward a multiple of 32) and, outside it, five Linears told apart by
shape: 1->64 (embedding), 1024->128, 128->64, 64->4 (actor), 64->1 (critic). ReLU / Sequential containers around them are
ignored; the forward pass is the reference's (embedding -> encoder -> flatten -> fc1 + ReLU -> fc2 + ReLU -> softmax(actor),
critic). Anything else raises ValueError with the reason; a module in training mode is refused (dropout has no device
counterpart).
"""
import torch

from . import _encoder_net as E
from . import ops
from ._encoder_net import flatten, unflatten        # noqa: F401 -- over this module's Parsed

NAME = "DeviceTransformerPolicy"
D_MODEL, N_HEAD, TOKENS = 64, 4, 16
_ROLES = {(1, 64): "embedding", (1024, 128): "fc1", (128, 64): "fc2", (64, 4): "actor", (64, 1): "critic"}


class Parsed:
    """The module's parts: embedding, layers (TransformerEncoderLayer list), fc1, fc2, actor, critic, dim_ff."""
    __slots__ = ("embedding", "layers", "fc1", "fc2", "actor", "critic", "dim_ff")
    name = NAME

    def plain_tensors(p):
        """The parameters in the order of g2048_tpolicy_pack's plain layout (LayerNorm eps as Python floats)."""
        return ([p.embedding.weight, p.embedding.bias] + E.layer_tensors(p.layers) +
                [p.fc1.weight, p.fc1.bias, p.fc2.weight, p.fc2.bias, p.actor.weight, p.actor.bias, p.critic.weight, p.critic.bias])


plain_tensors = Parsed.plain_tensors


def parse(module):
    """The module as a Parsed record. Raises ValueError naming the reason."""
    enc = E.find_encoder(NAME, module)
    out = Parsed()
    E.claim_by_shape(NAME, module, enc, out, _ROLES)
    out.layers, out.dim_ff = E.checked_layers(NAME, enc, D_MODEL, nhead=N_HEAD, batch_first=True)
    return out


@torch.no_grad()
def forward_reference(p, boards, dtype=torch.float64, round_weights=None):
    """The parsed network on uint8 (N,16) boards with plain torch ops in `dtype` (any device): the yardstick of the kernel.
    round_weights: an optional function applied to every parameter first (e.g. a bf16 round trip)."""
    w = E.weight_caster(dtype, round_weights)
    x = boards.to(dtype) / 15
    x = x.reshape(-1, TOKENS, 1) * w(p.embedding.weight).reshape(1, 1, -1) + w(p.embedding.bias)
    n = x.shape[0]
    for lay in p.layers:
        a = lay.self_attn
        qkv = x @ w(a.in_proj_weight).T + w(a.in_proj_bias)
        q, k, v = (t.reshape(n, TOKENS, N_HEAD, -1).transpose(1, 2) for t in qkv.split(D_MODEL, -1))
        s = torch.softmax((q @ k.transpose(-1, -2)) / 4, -1)
        x = E.post_norm_tail(lay, x, (s @ v).transpose(1, 2).reshape(n, TOKENS, D_MODEL), w)
    h = torch.relu(x.reshape(n, -1) @ w(p.fc1.weight).T + w(p.fc1.bias))
    h = torch.relu(h @ w(p.fc2.weight).T + w(p.fc2.bias))
    return torch.softmax(h @ w(p.actor.weight).T + w(p.actor.bias), -1), h @ w(p.critic.weight).T + w(p.critic.bias)


def _check_loss_inputs(n, actions, old_log_probs, advantages, returns):
    for name, t, dtype in (("actions", actions, torch.int64), ("old_log_probs", old_log_probs, torch.float32),
                           ("advantages", advantages, torch.float32), ("returns", returns, torch.float32)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch.Tensor" % (NAME, name))
        if t.dtype != dtype:
            raise TypeError("%s: %s must be %s (got %s)" % (NAME, name, dtype, t.dtype))
        if tuple(t.shape) != (n,):
            raise ValueError("%s: %s must have shape (%d,), one entry per board (got %s)" % (NAME, name, n, tuple(t.shape)))


F32_EPS = float(torch.finfo(torch.float32).eps)


def rnd(t):
    """t as float32 (round to nearest even), then as bfloat16 (round to nearest even), back in t's dtype: the rounding of the bf16
    gradient pass (include/g2048_tbf16.h)."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


class _RoundedLinear(torch.autograd.Function):
    """y = rnd(x) rnd(W)^T + b as the bf16 pass computes it, forward and backward: dx = rnd(dy) rnd(W), dW = rnd(dy)^T rnd(x), and
    db = the sum of dy as the pass stores it -- rounded for linear1 (its dy is the bf16 dh), as it arrives for linear2."""

    @staticmethod
    def forward(ctx, x, weight, bias, stored_dy_is_bf16):
        xr, wr = rnd(x), rnd(weight)
        ctx.save_for_backward(xr, wr)
        ctx.stored_dy_is_bf16 = stored_dy_is_bf16
        return xr @ wr.T + bias

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        g = rnd(dy)
        stored = g if ctx.stored_dy_is_bf16 else dy
        return (g @ wr, g.reshape(-1, g.shape[-1]).T @ xr.reshape(-1, xr.shape[-1]), stored.reshape(-1, stored.shape[-1]).sum(0), None)


class _StoredBf16(torch.autograd.Function):
    """The hidden layer as the bf16 pass keeps it: rnd(v) forward; the gradient passes as it is (it is rounded where linear1's
    backward reads it, after the ReLU mask and the site-2 multiplier)."""

    @staticmethod
    def forward(ctx, v):
        return rnd(v)

    @staticmethod
    def backward(ctx, g):
        return g


def _feed_forward_bf16(x, w1, b1, w2, b2, m2):
    h = _StoredBf16.apply(m2(torch.relu(_RoundedLinear.apply(x, w1, b1, True))))
    return _RoundedLinear.apply(h, w2, b2, False)


def loss_grad_reference(p, boards, actions, old_log_probs, advantages, returns, clip_epsilon=0.3, value_coef=0.4, entropy_coef=0.05,
                        dtype=torch.float64, eps=F32_EPS, multipliers=None, ff_bf16=False):
    """PPOAgent.update()'s loss (agents/ppo_agent.py:378-400) on the parsed module's two heads, in eval mode, with plain torch ops
    in `dtype` and autograd over the ops of forward_reference. multipliers: None, or a callable (layer, site, shape, dtype) -> the
    dropout multipliers (keep x 1 / (1 - p)) of site 0 (the attention probabilities, (N,4,16,16)), 1 (dropout1, (N,16,64)), 2 (the
    hidden layer, (N,16,dim_ff)) or 3 (dropout2, (N,16,64)) of encoder layer `layer`: with it the function is the TRAINING-mode
    module's under those masks.
        logp = log(probs[i, actions[i]]), ratio = exp(logp - old_log_probs),
        actor = -mean(min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv)), vloss = mean((value[:, 0] - returns)^2),
        ent = mean(Categorical(probs).entropy()), loss = actor + value_coef vloss - entropy_coef ent.
    Categorical(probs=probs) renormalises and clamps the probabilities to [eps, 1 - eps]; eps defaults to float32's, which is what
    the float32 module and the kernel clamp at, whatever `dtype` is. Returns (losses (4,) = loss, actor, vloss, ent; probs (N,4);
    value (N,1); grad: d loss / d parameter flat in the plain layout, the LayerNorm-eps slots 0). The yardstick of
    g2048_tpolicy_loss_grad; the module's own .grad fields are not touched. ff_bf16: the function of the bf16 gradient pass
    (grad_precision="bf16", include/g2048_tbf16.h) restated in `dtype`: every operand of a layer's feed-forward products rounded by
    rnd, the hidden layer and its gradient kept rounded, linear1's bias gradient the sum of the rounded dh; it composes with
    multipliers. False, the default: what the function returned before it had the argument."""
    n = boards.shape[0]
    _check_loss_inputs(n, actions, old_log_probs, advantages, returns)
    seq = p.plain_tensors()
    params = [t for t in seq if isinstance(t, torch.Tensor)]
    leaf = {id(t): t.detach().to(dtype).requires_grad_(True) for t in params}
    w = lambda t: leaf[id(t)]       # noqa: E731
    with torch.enable_grad():
        x = boards.to(dtype) / 15
        x = x.reshape(-1, TOKENS, 1) * w(p.embedding.weight).reshape(1, 1, -1) + w(p.embedding.bias)
        for i, lay in enumerate(p.layers):
            a = lay.self_attn
            mult = None if multipliers is None else (lambda site, shape, dt, i=i: multipliers(i, site, shape, dt))
            qkv = x @ w(a.in_proj_weight).T + w(a.in_proj_bias)
            q, k, v = (t.reshape(n, TOKENS, N_HEAD, -1).transpose(1, 2) for t in qkv.split(D_MODEL, -1))
            s = torch.softmax((q @ k.transpose(-1, -2)) / 4, -1)
            if mult is not None:
                s = s * mult(0, tuple(s.shape), s.dtype)
            x = E.post_norm_tail(lay, x, (s @ v).transpose(1, 2).reshape(n, TOKENS, D_MODEL), w, mult, _feed_forward_bf16 if ff_bf16 else None)
        h = torch.relu(x.reshape(n, -1) @ w(p.fc1.weight).T + w(p.fc1.bias))
        h = torch.relu(h @ w(p.fc2.weight).T + w(p.fc2.bias))
        probs = torch.softmax(h @ w(p.actor.weight).T + w(p.actor.bias), -1)
        value = h @ w(p.critic.weight).T + w(p.critic.bias)
        qn = probs / probs.sum(-1, keepdim=True)
        logits = torch.log(torch.clamp(qn, min=eps, max=1 - eps))
        logp = logits.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
        ent = -(logits * qn).sum(-1).mean()
        ratio = torch.exp(logp - old_log_probs.to(dtype))
        adv = advantages.to(dtype)
        actor = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip_epsilon, 1 + clip_epsilon) * adv).mean()
        vloss = ((value[:, 0] - returns.to(dtype)) ** 2).mean()
        loss = actor + value_coef * vloss - entropy_coef * ent
        grads = dict(zip((id(t) for t in params), torch.autograd.grad(loss, [leaf[id(t)] for t in params])))
    flat = torch.cat([grads[id(t)].reshape(-1) if isinstance(t, torch.Tensor) else torch.zeros(1, dtype=dtype, device=boards.device)
                      for t in seq])
    return torch.stack([loss, actor, vloss, ent]).detach(), probs.detach(), value.detach(), flat


def _loss_outputs(n, device):       # losses, probs, value
    return (torch.empty(4, dtype=torch.float32, device=device), torch.empty((n, 4), dtype=torch.float32, device=device),
            torch.empty((n, 1), dtype=torch.float32, device=device))


def _advantage_buffers(n, device):  # the two forwards' probabilities (not returned), value, next value, returns, advantages
    return (torch.empty((n, 4), dtype=torch.float32, device=device),) + tuple(
        torch.empty(shape, dtype=torch.float32, device=device) for shape in ((n, 1), (n, 1), (n,), (n,)))


def _norm_out(n, device):           # adam_step's gradient norm
    return torch.empty((), dtype=torch.float32, device=device)


def _update_outputs(epochs, device):        # update()'s losses and norms, a row an epoch
    return torch.empty((epochs, 4), dtype=torch.float32, device=device), torch.empty(epochs, dtype=torch.float32, device=device)


def _outputs(n, device):
    return torch.empty((n, 4), dtype=torch.float32, device=device), torch.empty((n, 1), dtype=torch.float32, device=device)


class DeviceTransformerPolicy(E.PackedNet):
    """Transformer policy on the device: __call__(boards uint8 (N,16)) -> (probs float32 (N,4), value float32 (N,1)). One
    g2048_tpolicy_forward launch per call; the outputs are buffers owned by the policy (one pair per (N, stream), overwritten
    by the next call with the same N on the same stream), so after the first call per (N, stream) a call neither allocates nor
    synchronises and can be captured in a graph (RolloutCollector does).

    precision: "f32" (exact f32 MFMA, the parity path) or "bf16" (bf16 weights and matmul inputs, f32 accumulation, LayerNorm,
    softmax and attention products).
    refresh() re-flattens and re-packs the weights IN PLACE on the current stream (call it after an optimizer step; the module
    must be back in eval mode): graphs captured earlier replay with the new weights. After attach_params() the module IS the
    plain buffer and refresh() only packs.
    loss_and_grad(...) fills net.grad; attach_grads() / attach_params() hand both buffers to a stock optimizer as views.
    adam_step(losses) is the rest of a PPO epoch on the device (NaN gate, clipping, Adam: net.exp_avg, net.exp_avg_sq,
    net.opt_counters), update(...) the whole of PPOAgent.update() after its sampling without a host read, and
    optimizer_state_dict() / load_optimizer_state_dict() exchange the state with torch.optim.Adam(model.parameters()).
    dropout, dropout_seed: what the TRAINING forwards apply (loss_and_grad, advantages, update); the module docstring. 0.0, the
    default: none, through the entry points and with the bits of a policy built without the argument.
    grad_precision: "f32" (the default: the gradient pass as ever, bit for bit) or "bf16": loss_and_grad and update run the seven
    feed-forward products of every encoder layer on the bf16 matrix cores (include/g2048_tbf16.h). advantages(), the acting
    forward and the optimiser step are the same either way. Any other value raises ValueError.

    takes_boards = True: RolloutCollector hands it the packed boards instead of the float observations."""

    takes_boards = True
    name, parse = NAME, staticmethod(parse)
    plain_floats, packed_bytes, pack = map(staticmethod, (ops.tpolicy_plain_floats, ops.tpolicy_packed_bytes, ops.tpolicy_pack))

    def __init__(self, model, precision="f32", dropout=0.0, dropout_seed=0, grad_precision="f32"):
        self.grad_precision = ops.check_grad_precision(grad_precision)
        self.dropout = E.dropout_of(NAME, parse(model), dropout)    # (attention, dropout1, dropout, dropout2)
        self.dropout_seed, self.dropout_index = ops.L.u64(dropout_seed), 0
        super().__init__(model, precision)

    def dropout_state(self):
        """(dropout_seed, dropout_index): with the weights, what reproduces the masks of every later training forward."""
        return self.dropout_seed, self.dropout_index

    def set_dropout_state(self, state):
        seed, index = state
        if int(index) < 0:
            raise ValueError("%s: the dropout index must not be negative" % NAME)
        self.dropout_seed, self.dropout_index = ops.L.u64(seed), int(index)

    def _next_index(self):
        index = self.dropout_index
        self.dropout_index = index + 1
        return index

    def __call__(self, boards):
        probs, value = self._out.get(self._out.rows(boards), _outputs)
        return ops.tpolicy_forward(boards, self.packed, self.dim_ff, self.n_layers, self.precision, probs=probs, value=value)

    def _grad_workspace(self, n, device):           # refuses n = 0 and n above the maximum
        return torch.empty(ops.tpolicy_grad_workspace_bytes(n, self.dim_ff, self.n_layers), dtype=torch.uint8, device=device)

    def _train_workspace(self, n, device):          # the training passes': one more array
        return torch.empty(ops.tpolicy_train_workspace_bytes(n, self.dim_ff, self.n_layers), dtype=torch.uint8, device=device)

    def _bf16_workspace(self, n, device):           # the bf16 gradient pass's: the hidden layer and its gradient at 2 bytes
        return torch.empty(ops.tpolicy_bf16_workspace_bytes(n, self.dim_ff, self.n_layers), dtype=torch.uint8, device=device)

    def loss_and_grad(self, boards, actions, old_log_probs, advantages, returns, clip_epsilon=0.3, value_coef=0.4, entropy_coef=0.05):
        """(losses float32 (4,) = loss, actor loss, value loss, entropy; probs float32 (N,4); value float32 (N,1)) of
        PPOAgent.update()'s loss (agents/ppo_agent.py:378-400; the coefficients default to PPOAgent's) on uint8 (N,16) boards,
        int64 (N,) actions and float32 (N,) old_log_probs, advantages and returns, the module in eval mode; net.grad is
        OVERWRITTEN with d loss / d parameter in the layout of net.plain (g2048_tpolicy_loss_grad: the forward with its
        activations kept, the loss head, the backward, one phase per launch; no host synchronisation). 1 <= N <= 1024. The pass
        is f32 and reads net.plain, whatever precision the acting blob is packed in. An action outside 0..3 is the caller's
        error (the kernel reads actions & 3). The outputs and the workspace are the network's (one set per (N, stream)): after
        the first call per (N, stream) nothing is allocated. This is a training forward: with any net.dropout > 0 it is the
        module's TRAINING-mode pass (g2048_tpolicy_loss_grad_dropout) under the masks of (net.dropout_seed, net.dropout_index),
        regenerated in the backward; the index counts on either way, and with dropout 0 the call and its bits are as ever. With
        net.grad_precision "bf16" the feed-forward products of every encoder layer take bf16 operands and the hidden layer is kept
        as bf16 (g2048_tpolicy_loss_grad_bf16, with or without dropout): gradients then differ from the f32 pass's by per cents of
        their largest element, not by rounding (docs/LOG.md R37); net.plain, net.grad and the step stay f32."""
        return self._loss_and_grad(boards, actions, old_log_probs, advantages, returns, clip_epsilon, value_coef, entropy_coef, None)

    def _loss_and_grad(self, boards, actions, old_log_probs, advantages, returns, clip_epsilon, value_coef, entropy_coef, losses_row):
        if not isinstance(boards, torch.Tensor) or boards.dim() != 2:
            raise TypeError("%s.loss_and_grad: boards must be a uint8 (N,16) tensor" % NAME)
        _check_loss_inputs(boards.shape[0], actions, old_log_probs, advantages, returns)
        n = self._out.rows(boards)
        if n > ops.L.TLEARN_BATCH_MAX:
            raise ValueError("%s.loss_and_grad: takes at most %d boards a call (16,384 tokens), got %d; a larger batch is refused, not "
                             "truncated" % (NAME, ops.L.TLEARN_BATCH_MAX, n))
        losses, probs, value = self._out.get(n, _loss_outputs)
        if losses_row is not None:              # update(): the epoch's row of its own losses tensor
            losses = losses_row
        ops.tpolicy_loss_grad(boards, self.plain, actions, old_log_probs, advantages, returns, self.dim_ff, self.n_layers, clip_epsilon,
                              value_coef, entropy_coef, grad=self.grad, losses=losses, probs=probs, value=value,
                              workspace=self._out.get(n, self._bf16_workspace if self.grad_precision == "bf16" else
                                                      self._train_workspace if any(self.dropout) else self._grad_workspace) if n else None,
                              dropout=self.dropout, seed=self.dropout_seed, call_index=self._next_index(), grad_precision=self.grad_precision)
        return losses, probs, value

    def advantages(self, boards, next_boards, rewards, dones, gamma=0.995, training=None):
        """(returns, advantages) float32 (N,) of PPOAgent.update()'s first block (agents/ppo_agent.py:357-373) with this network's
        critic head: two f32 forwards (through a blob packed from net.plain at f32: the acting blob when precision is "f32"),
        returns = rewards + gamma * value(next_boards) * (1 - dones), advantages = returns - value(boards), normalised by their
        mean and unbiased std (+ 1e-8) when N > 1 (g2048_ppo_advantages). rewards, dones float32 (N,). The outputs are the
        network's (one pair per (N, stream)); no synchronisation. training: None means training iff any net.dropout > 0. Training
        is the reference's block with the network in training mode: two g2048_tpolicy_forward_dropout calls from net.plain, boards
        first and then next_boards, with two consecutive dropout indices (1 <= N <= 1024). Otherwise the two fused eval-mode
        forwards run, and the index stays."""
        n = self._out.rows(boards)
        if self._out.rows(next_boards) != n:
            raise ValueError("%s.advantages: boards and next_boards must have the same number of rows" % NAME)
        if any(self.dropout) if training is None else training:
            probs, value, next_value, returns, adv = self._out.get(n, _advantage_buffers)
            workspace = self._out.get(n, self._train_workspace) if n else None
            for b, v in ((boards, value), (next_boards, next_value)):
                ops.tpolicy_forward_train(b, self.plain, self.dim_ff, self.n_layers, self.dropout, self.dropout_seed, self._next_index(),
                                          probs=probs, value=v, workspace=workspace)
            return ops.ppo_advantages(value, next_value, rewards, dones, gamma, returns=returns, advantages=adv)
        packed = self.packed
        if self.precision != "f32":
            packed = self._out.get(0, self._f32_blob)
            self.pack(self.plain, self.dim_ff, self.n_layers, "f32", out=packed)
        probs, value, next_value, returns, adv = self._out.get(n, _advantage_buffers)
        ops.tpolicy_forward(boards, packed, self.dim_ff, self.n_layers, "f32", probs=probs, value=value)
        ops.tpolicy_forward(next_boards, packed, self.dim_ff, self.n_layers, "f32", probs=probs, value=next_value)
        return ops.ppo_advantages(value, next_value, rewards, dones, gamma, returns=returns, advantages=adv)

    def _f32_blob(self, n, device):
        return torch.empty(self.packed_bytes("f32", self.dim_ff, self.n_layers), dtype=torch.uint8, device=device)

    # ---- the optimiser's side: the NaN gate, clipping and Adam on the device (g2048_tpolicy_adam_step, the step library)
    _hyper = (3e-4, (0.9, 0.999), 1e-8)     # the last adam_step's lr, betas, eps: optimizer_state_dict's group

    @property
    def opt_counters(self):
        """int64 (3,) on the device: {Adam steps applied, calls skipped for a NaN loss, calls skipped for a gradient norm that is
        not finite} (zeros, allocated on first use). opt_counters[0] is the step number of Adam's bias correction."""
        c = self.__dict__.get("_opt_counters")
        if c is None:
            c = self.__dict__["_opt_counters"] = torch.zeros(3, dtype=torch.int64, device=self.device)
        return c

    def _step_workspace(self, n, device):
        return torch.empty(ops.tpolicy_step_workspace_bytes(self.dim_ff, self.n_layers), dtype=torch.uint8, device=device)

    def _adam_step(self, losses, lr, max_norm, betas, eps, norm):
        ops.tpolicy_adam_step(self.plain, self.grad, self.exp_avg, self.exp_avg_sq, self.dim_ff, self.n_layers, self.opt_counters,
                              losses=losses, lr=lr, betas=betas, eps=eps, max_norm=max_norm, norm=norm,
                              workspace=self._out.get(0, self._step_workspace))
        self._hyper = (lr, betas, eps)          # as given (tpolicy_adam_step accepted them); optimizer_state_dict reads them
        return norm

    def adam_step(self, losses=None, lr=3e-4, max_norm=0.5, betas=(0.9, 0.999), eps=1e-8):
        """The end of an epoch of PPOAgent.update (agents/ppo_agent.py:403-416) on the device, after loss_and_grad: the NaN check
        on losses[0] (losses: what loss_and_grad returned; None: no check), clip_grad_norm_(max_norm) and an Adam step, in three
        launches (g2048_tpolicy_adam_step). net.plain is updated IN PLACE from net.grad (left clipped, as clip_grad_norm_ leaves
        it), the moments are net.exp_avg and net.exp_avg_sq. max_norm None: no clipping. The reference never trains this model,
        so lr has no reference value: 3e-4 is examples/tpolicy_update.py's default; max_norm, betas and eps are PPOAgent's. A NaN
        loss, or a gradient norm that is not finite, skips the call: no buffer changes, and opt_counters[1] or [2] counts it;
        otherwise opt_counters[0] goes up by one and is the step number of Adam's bias correction, read on the device (a skipped
        call does not advance it). The LayerNorm-eps slots are settings and are not updated. Works for both precisions: the
        pass and the step are f32 on net.plain. The call ends by packing net.plain into net.packed IN PLACE at the network's
        precision (a forward captured earlier in a graph replays with the new weights) and loads the module's parameters from
        net.plain unless attach_params() made them views of it. Returns the norm before clipping as a float32 () device tensor
        (the network's own, one per stream; written on a skipped call too), without synchronising."""
        norm = self._adam_step(losses, lr, max_norm, betas, eps, self._out.get(0, _norm_out))
        self._plain_changed()
        return norm

    def update(self, boards, actions, old_log_probs, rewards, next_boards, dones, epochs=8, gamma=0.995, **adam):
        """PPOAgent.update() after its sampling (agents/ppo_agent.py:357-416) for this network on the device: advantages(boards,
        next_boards, rewards, dones, gamma), then `epochs` times loss_and_grad (PPOAgent's coefficients) and the step on that
        epoch's losses (**adam: adam_step's lr, max_norm, betas, eps), then ONE pack of net.packed and one write-back of the
        module. A sequence of launches with no host decision and no host read: an epoch whose loss is a NaN or whose gradient is
        not finite is skipped on the device and shows in opt_counters and in the returned rows. Returns (losses float32
        (epochs,4), norms float32 (epochs,)), device tensors the network owns (one pair per (epochs, stream)): row e is epoch e's
        loss_and_grad result and its gradient norm before clipping. With dropout one update uses 2 + epochs consecutive dropout
        indices, in that order (the advantage block's two forwards, then the epochs), still with no host read. A captured graph of
        update() replays the masks it was captured with: the indices are kernel arguments, as for DevicePPOLearner."""
        epochs = int(epochs)
        if epochs < 1:
            raise ValueError("%s: update needs at least one epoch" % NAME)
        unknown = set(adam) - {"lr", "max_norm", "betas", "eps"}
        if unknown:
            raise TypeError("%s: update got unexpected arguments %s" % (NAME, sorted(unknown)))
        adam = dict(dict(lr=3e-4, max_norm=0.5, betas=(0.9, 0.999), eps=1e-8), **adam)
        returns, adv = self.advantages(boards, next_boards, rewards, dones, gamma)
        losses, norms = self._out.get(epochs, _update_outputs)
        for e in range(epochs):
            self._loss_and_grad(boards, actions, old_log_probs, adv, returns, 0.3, 0.4, 0.05, losses[e])
            self._adam_step(losses[e], adam["lr"], adam["max_norm"], adam["betas"], adam["eps"], norms[e])
        self._plain_changed()
        return losses, norms

    def _param_offsets(self):
        """[(parameter, offset in floats into net.plain)] in model.parameters() order: the module is recognised by structure, so
        that order need not be the plain order; each parameter is found in the plain layout by identity."""
        at, o = {}, 0
        for t in self.parsed.plain_tensors():
            if isinstance(t, torch.Tensor):
                at[id(t)] = o
                o += t.numel()
            else:
                o += 1
        params = list(self.model.parameters())
        if len(params) != len(at) or any(id(p) not in at for p in params):
            raise ValueError("%s: model.parameters() are not the %d tensors of the plain layout" % (NAME, len(at)))
        return [(p, at[id(p)]) for p in params]

    def optimizer_state_dict(self):
        """The state of adam_step's Adam in the format torch.optim.Adam(model.parameters()).state_dict() has: an entry per
        parameter in model.parameters() order, each {step, exp_avg, exp_avg_sq} (copies, shaped like the parameter; step is
        opt_counters' applied-step count), and one parameter group holding the last adam_step's lr, betas and eps (adam_step's
        defaults before the first call). Before the first applied step the state is empty, as a fresh optimiser's is. A stock
        optimiser's load_state_dict takes it as it is. Synchronises (it reads the counter)."""
        lr, betas, eps = self._hyper
        group = torch.optim.Adam([torch.nn.Parameter(torch.zeros(()))], lr=float(lr), betas=(float(betas[0]), float(betas[1])),
                                 eps=float(eps)).state_dict()["param_groups"][0]
        pairs = self._param_offsets()
        group["params"] = list(range(len(pairs)))
        step, state = int(self.opt_counters[0]), {}
        if step > 0:
            for i, (p, o) in enumerate(pairs):
                state[i] = dict(step=torch.tensor(float(step)), exp_avg=self.exp_avg[o:o + p.numel()].view(p.shape).clone(),
                                exp_avg_sq=self.exp_avg_sq[o:o + p.numel()].view(p.shape).clone())
        return dict(state=state, param_groups=[group])

    @torch.no_grad()
    def load_optimizer_state_dict(self, state_dict):
        """Takes what torch.optim.Adam(model.parameters()).state_dict() (or optimizer_state_dict) gave: the moments into exp_avg
        and exp_avg_sq at each parameter's place in the plain layout, the step into opt_counters[0] (the skip counts stay). An
        empty state resets moments and step to 0. The group's lr, betas and eps are NOT taken: they are adam_step's arguments.
        amsgrad, maximize and a weight decay are refused: adam_step is plain Adam. The LayerNorm-eps slots of the moments are not
        written."""
        pairs = self._param_offsets()
        groups, state = state_dict["param_groups"], state_dict["state"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(pairs):
            raise ValueError("%s: expected one parameter group of %d parameters (torch.optim.Adam(model.parameters()))" % (NAME, len(pairs)))
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize") or g.get("weight_decay", 0) != 0:
            raise ValueError("%s: amsgrad, maximize and weight_decay are not what adam_step computes" % NAME)
        if not state:
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            self.opt_counters[0] = 0
            return
        keys = list(g["params"])
        if set(state) != set(keys):
            raise ValueError("%s: the state must hold all %d parameters or none" % (NAME, len(keys)))
        steps = {int(state[key]["step"]) for key in keys}
        if len(steps) != 1 or min(steps) < 0:
            raise ValueError("%s: the parameters' step counts differ or are negative: %s" % (NAME, sorted(steps)))
        for key, (p, _) in zip(keys, pairs):
            for name in ("exp_avg", "exp_avg_sq"):
                if tuple(state[key][name].shape) != tuple(p.shape):
                    raise ValueError("%s: %s of parameter %s has shape %s, the parameter %s"
                                     % (NAME, name, key, tuple(state[key][name].shape), tuple(p.shape)))
        for key, (p, o) in zip(keys, pairs):
            self.exp_avg[o:o + p.numel()].copy_(state[key]["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + p.numel()].copy_(state[key]["exp_avg_sq"].reshape(-1))
        self.opt_counters[0] = steps.pop()
