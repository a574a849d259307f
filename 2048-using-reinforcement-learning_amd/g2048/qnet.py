"""The hybrid agent's CNN-transformer Q-network (agents/hybrid.py:700-727, HybridDQN, eval mode) as one HIP launch on the
packed boards.

`DeviceQNetwork(model, precision="f32")` takes a torch module of that structure, flattens its parameters into the plain layout
of include/g2048.h (state-dict order, plus the two LayerNorm eps per layer), packs them with `g2048_qnet_pack` and runs
`g2048_qnet_forward` on uint8 (N,16) boards.

Per-board semantics. The reference's encoder layer is not batch_first and is fed x.unsqueeze(1), so model(x) on a batch of B
boards is ONE sequence of B tokens that attend to each other; the reference only ever calls it with one board. Row i here is
model(x[i:i+1]): every board is a sequence of one token, the attention softmax is exactly 1.0 and the attention block is
out_proj(W_v x + b_v). Q, K, the head count and batch_first cannot influence that and are not constrained. The reference never
calls .eval() (its dropout is live even in select_action); acting here -- __call__, act, act_beam, the play kernels -- is the
eval-mode function, dropout in select_action being an accident of the reference.

Training. DQNAgent.train_step's three forwards (hybrid.py:1038, :1042, :1044) run nn.TransformerEncoderLayer's four dropout sites
live, and so do the training forwards here when the network is built with `dropout`: DeviceQNetwork(model, dropout=0.1 | (p_attention,
p_dropout1, p_dropout, p_dropout2) | "module", dropout_seed=s). loss_and_grad applies it, forward_batch(boards, training=True) and
dqn_targets(..., training=True) apply it; forward_batch(boards) stays eval mode. The masks are counter-RNG draws (include/g2048_train.h;
ops.qnet_dropout_mask writes a site's keep bits), regenerated in the backward pass instead of stored. `dropout_index` is the call
index of the NEXT training forward, a Python int counted on the host (it counts with dropout 0 too); dropout_state() /
set_dropout_state() carry (seed, index) through a checkpoint. The index is a launch scalar: a captured graph replays the SAME masks
on every replay. sync_from copies weights only: give the online and the target network different seeds, as the reference's two
modules draw independently; with the same seed and index their masks coincide. With dropout 0, the default, every call goes
through the main library's entry points and gives the bits it always gave.

The module is recognised by structure, not by attribute names: two Conv2d (1->32 and 32->64, kernel 2, stride 1, paddings 1 and
0), exactly one nn.TransformerEncoder (post-norm ReLU layers, d_model 128, no final norm, dim_feedforward a multiple of 32) and,
outside it, two Linears told apart by shape: 1024->128 (embedding) and 128->4 (fc). ReLU / Sequential containers around them are
ignored. Anything else raises ValueError with the reason; a module in training mode is refused at construction and in
refresh() (what the training forwards apply is the `dropout` argument's business, not the module's mode).
"""
import torch
import torch.nn.functional as F

from . import _encoder_net as E
from . import ops
from ._encoder_net import flatten, unflatten        # noqa: F401 -- over this module's Parsed

NAME = "DeviceQNetwork"
D_MODEL = 128
_ROLES = {(1024, 128): "embedding", (128, 4): "fc"}
_CONVS = {(1, 32): "conv1", (32, 64): "conv2"}                     # by (in, out) channels
_PADDING = {"conv1": 1, "conv2": 0}


class Parsed:
    """The module's parts: conv1, conv2, embedding, layers (TransformerEncoderLayer list), fc, dim_ff; nhead and batch_first are
    tuples with one entry per layer (they matter to forward_batch only)."""
    __slots__ = ("conv1", "conv2", "embedding", "layers", "fc", "dim_ff", "nhead", "batch_first")
    name = NAME

    def plain_tensors(p):
        """The parameters in the order of g2048_qnet_pack's plain layout (LayerNorm eps as Python floats)."""
        return ([p.conv1.weight, p.conv1.bias, p.conv2.weight, p.conv2.bias, p.embedding.weight, p.embedding.bias] +
                E.layer_tensors(p.layers) + [p.fc.weight, p.fc.bias])


plain_tensors = Parsed.plain_tensors


def _check_conv(m, role, what):
    pad = _PADDING[role]
    if tuple(m.kernel_size) != (2, 2) or tuple(m.stride) != (1, 1):
        E._refuse(NAME, "the %s needs kernel 2 and stride 1 (got kernel %s, stride %s)" % (what, tuple(m.kernel_size), tuple(m.stride)))
    if m.padding != (pad, pad) or m.padding_mode != "zeros":
        E._refuse(NAME, "the %s needs zero padding %d (got %s, %s)" % (what, pad, m.padding, m.padding_mode))
    if tuple(m.dilation) != (1, 1) or m.groups != 1:
        E._refuse(NAME, "the %s has dilation or groups other than 1" % what)
    if m.bias is None:
        E._refuse(NAME, "the %s has a missing bias" % what)


def parse(module):
    """The module as a Parsed record. Raises ValueError naming the reason."""
    enc = E.find_encoder(NAME, module)
    out = Parsed()
    E.claim_by_shape(NAME, module, enc, out, _ROLES, _CONVS, _check_conv)
    out.layers, out.dim_ff = E.checked_layers(NAME, enc, D_MODEL)
    out.nhead = tuple(int(lay.self_attn.num_heads) for lay in out.layers)
    out.batch_first = tuple(bool(lay.self_attn.batch_first) for lay in out.layers)
    return out


def tile_values(boards, dtype=torch.float64):
    """uint8 (N,16) codes as the env's get_state(): 2 ** code, 0 for an empty cell."""
    c = boards.to(torch.int64)
    return torch.where(c > 0, torch.ones_like(c) << c, torch.zeros_like(c)).to(dtype)


@torch.no_grad()
def forward_reference(p, boards, dtype=torch.float64, round_weights=None):
    """Q (N,4) of the parsed network on uint8 (N,16) boards with plain torch ops in `dtype` (any device), every board its own
    sequence of one token: the yardstick of the kernel. round_weights: an optional function applied to every parameter first
    (e.g. a bf16 round trip)."""
    w = E.weight_caster(dtype, round_weights)
    x = tile_values(boards, dtype).reshape(-1, 1, 4, 4)
    x = torch.relu(F.conv2d(x, w(p.conv1.weight), w(p.conv1.bias), padding=1))
    x = torch.relu(F.conv2d(x, w(p.conv2.weight), w(p.conv2.bias)))
    x = x.reshape(x.shape[0], -1) @ w(p.embedding.weight).T + w(p.embedding.bias)
    for lay in p.layers:
        a = lay.self_attn
        x = E.post_norm_tail(lay, x, x @ w(a.in_proj_weight)[2 * D_MODEL:].T + w(a.in_proj_bias)[2 * D_MODEL:], w)
    return x @ w(p.fc.weight).T + w(p.fc.bias)


NHEAD = 8


def check_batch_layers(p):
    """forward_batch's constraints on the parsed module's layers: one sequence of tokens that attend to each other, 8 heads."""
    for i, (h, bf) in enumerate(zip(p.nhead, p.batch_first)):
        if bf:
            E._refuse(NAME, "forward_batch: encoder layer %d has batch_first=True: the module's own batch call is then the per-board "
                            "function, which __call__ computes" % i)
        if h != NHEAD:
            E._refuse(NAME, "forward_batch: encoder layer %d has nhead %d, expected %d (the attention kernel is built for 8 heads of 16)"
                      % (i, h, NHEAD))


@torch.no_grad()
def forward_batch_reference(p, boards, dtype=torch.float64):
    """Q (N,4) of the parsed network on uint8 (N,16) boards as ONE call of the module in eval mode, with plain torch ops in `dtype`
    (any device): the N boards are one sequence of N tokens that attend to each other (the encoder layer is not batch_first and
    sees x.unsqueeze(1)). Per layer the whole in_proj, 8 heads of 16, softmax(q.k / 4) over all N keys, P.V, then the post-norm
    tail. The yardstick of g2048_qnet_forward_batch; at N = 1 it is forward_reference."""
    check_batch_layers(p)
    w = E.weight_caster(dtype)
    n = boards.shape[0]
    x = tile_values(boards, dtype).reshape(-1, 1, 4, 4)
    x = torch.relu(F.conv2d(x, w(p.conv1.weight), w(p.conv1.bias), padding=1))
    x = torch.relu(F.conv2d(x, w(p.conv2.weight), w(p.conv2.bias)))
    x = x.reshape(n, -1) @ w(p.embedding.weight).T + w(p.embedding.bias)
    for lay in p.layers:
        a = lay.self_attn
        q, k, v = (x @ w(a.in_proj_weight).T + w(a.in_proj_bias)).split(D_MODEL, dim=1)
        head = D_MODEL // NHEAD
        q, k, v = (t.reshape(n, NHEAD, head).transpose(0, 1) for t in (q, k, v))            # (heads, N, 16)
        prob = torch.softmax(q @ k.transpose(1, 2) / (head ** 0.5), dim=-1)
        x = E.post_norm_tail(lay, x, (prob @ v).transpose(0, 1).reshape(n, D_MODEL), w)
    return x @ w(p.fc.weight).T + w(p.fc.bias)


def dropout_of(p, dropout):
    """The four dropout probabilities of DeviceQNetwork's `dropout` for the parsed module p (_encoder_net.dropout_of)."""
    return E.dropout_of(NAME, p, dropout)


def _check_loss_inputs(n, actions, targets, weights):
    for name, t, dtype in (("actions", actions, torch.int64), ("targets", targets, torch.float32), ("weights", weights, torch.float32)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch.Tensor" % (NAME, name))
        if t.dtype != dtype:
            raise TypeError("%s: %s must be %s (got %s)" % (NAME, name, dtype, t.dtype))
        if tuple(t.shape) != (n,):
            raise ValueError("%s: %s must have shape (%d,), one entry per board (got %s)" % (NAME, name, n, tuple(t.shape)))


def loss_grad_reference(p, boards, actions, targets, weights, dtype=torch.float64):
    """The gradient half of DQNAgent.train_step (hybrid.py:1038, :1049-1055) in eval mode with plain torch ops in `dtype`:
    autograd over the ops of forward_batch_reference, the Huber error of q[i, actions[i]] against targets[i]
    (nn.SmoothL1Loss(reduction='none'), beta 1) and loss = mean(weights * td). Returns (loss, td, q, grads): grads maps every
    parameter of the parsed module to its gradient, in the plain layout's order. The yardstick of g2048_qnet_loss_grad; the
    module's own .grad fields are not touched."""
    check_batch_layers(p)
    n = boards.shape[0]
    _check_loss_inputs(n, actions, targets, weights)
    params = [t for t in p.plain_tensors() if isinstance(t, torch.Tensor)]
    leaf = {id(t): t.detach().to(dtype).requires_grad_(True) for t in params}
    w = lambda t: leaf[id(t)]
    with torch.enable_grad():
        x = tile_values(boards, dtype).reshape(-1, 1, 4, 4)
        x = torch.relu(F.conv2d(x, w(p.conv1.weight), w(p.conv1.bias), padding=1))
        x = torch.relu(F.conv2d(x, w(p.conv2.weight), w(p.conv2.bias)))
        x = x.reshape(n, -1) @ w(p.embedding.weight).T + w(p.embedding.bias)
        for lay in p.layers:
            a = lay.self_attn
            q, k, v = (x @ w(a.in_proj_weight).T + w(a.in_proj_bias)).split(D_MODEL, dim=1)
            head = D_MODEL // NHEAD
            q, k, v = (t.reshape(n, NHEAD, head).transpose(0, 1) for t in (q, k, v))
            prob = torch.softmax(q @ k.transpose(1, 2) / (head ** 0.5), dim=-1)
            x = E.post_norm_tail(lay, x, (prob @ v).transpose(0, 1).reshape(n, D_MODEL), w)
        qv = x @ w(p.fc.weight).T + w(p.fc.bias)
        td = F.smooth_l1_loss(qv.gather(1, actions.unsqueeze(1)).squeeze(1), targets.to(dtype), reduction="none")
        loss = (weights.to(dtype) * td).mean()
        grads = torch.autograd.grad(loss, [leaf[id(t)] for t in params])
    return loss.detach(), td.detach(), qv.detach(), dict(zip(params, grads))


@torch.no_grad()
def adamw_step_reference(plain, grad, exp_avg, exp_avg_sq, eps_at, lr, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4,
                         max_norm=10.0, dtype=torch.float64):
    """clip_grad_norm_(max_norm) followed by AdamW.step() number `step` (>= 1) on flat buffers in the plain layout, with plain
    torch ops in `dtype` (any device): the yardstick of g2048_qnet_adamw_step. With norm = ||grad|| (summed in float64, then
    rounded to `dtype`) and c = min(1, max_norm / (norm + 1e-6)) (max_norm None: no clipping),
        g = grad c;  p = plain (1 - lr wd);  m = m + (g - m)(1 - beta1);  v = v beta2 + (g g)(1 - beta2);
        p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps)),  bc1 = 1 - beta1^step, bc2 = 1 - beta2^step,
    the scalars formed in Python floats as torch's AdamW forms them. eps_at: the offsets of the LayerNorm-eps slots, which are
    settings and keep their values in all four buffers. A norm that is not finite changes nothing. Returns new (plain, grad,
    exp_avg, exp_avg_sq, norm) in `dtype`; the arguments are not modified."""
    p0, g0, m0, v0 = (t.detach().to(dtype) for t in (plain, grad, exp_avg, exp_avg_sq))
    norm = torch.linalg.vector_norm(g0, dtype=torch.float64).to(dtype)         # summed in float64 whatever the dtype, as the kernel sums it
    if not bool(torch.isfinite(norm)):
        return p0.clone(), g0.clone(), m0.clone(), v0.clone(), norm
    beta1, beta2 = betas
    c = torch.clamp((norm + 1e-6).reciprocal() * (float("inf") if max_norm is None else max_norm), max=1.0)      # torch's max_norm / tensor
    g = g0 * c
    p = p0 * (1 - lr * weight_decay)
    m = m0 + (g - m0) * (1 - beta1)
    v = v0 * beta2 + (g * g) * (1 - beta2)
    p = p - (lr / (1 - beta1 ** step)) * (m / (v.sqrt() / (1 - beta2 ** step) ** 0.5 + eps))
    at = torch.as_tensor(list(eps_at), dtype=torch.int64, device=p.device)
    for new, old in ((p, p0), (g, g0), (m, m0), (v, v0)):
        new[at] = old[at]
    return p, g, m, v, norm


def _q_only(n, device):
    return torch.empty((n, 4), dtype=torch.float32, device=device)


def _loss_outputs(n, device):       # loss, td, q
    return (torch.empty((), dtype=torch.float32, device=device), torch.empty(n, dtype=torch.float32, device=device),
            torch.empty((n, 4), dtype=torch.float32, device=device))


def _targets(n, device):
    return torch.empty(n, dtype=torch.float32, device=device), torch.empty(n, dtype=torch.int64, device=device)


def _outputs(n, device):
    return torch.empty((n, 4), dtype=torch.float32, device=device), torch.empty(n, dtype=torch.uint8, device=device)


def _norm_out(n, device):         # the gradient norm of adamw_step
    return torch.empty((), dtype=torch.float32, device=device)


def _explored(n, device):
    return torch.empty(n, dtype=torch.uint8, device=device)


def _planned(n, device):
    return torch.empty(n, dtype=torch.uint8, device=device)


def _candidates(n, device):         # the 32 candidate boards of every board, their count per action, their Q-values
    return (torch.empty((n, 32, 16), dtype=torch.uint8, device=device), torch.empty((n, 4), dtype=torch.uint8, device=device),
            torch.empty((n * 32, 4), dtype=torch.float32, device=device))


class DeviceQNetwork(E.PackedNet):
    """Hybrid Q-network on the device: __call__(boards uint8 (N,16)) -> q float32 (N,4); act(boards) -> (actions uint8 (N,), q),
    the exploit action of DQNAgent.select_action (argmax of q over the env's valid moves, ties to the lowest index, 0 for a board
    with no valid move); act(boards, epsilon, seed, step_index, id_base) with epsilon > 0 is the whole epsilon-greedy
    select_action (one more launch); act_beam(...) is select_action with the reference's use_beam_search = True. One
    g2048_qnet_forward launch per call; the outputs are buffers owned by the network (one set per
    (N, stream), overwritten by the next call with the same N on the same stream), so after the first call per (N, stream) a
    call neither allocates nor synchronises.

    precision: "f32" (exact f32 MFMA, the parity path) or "bf16" (bf16 weights and matmul inputs, f32 accumulation, biases,
    LayerNorm and residual adds).
    refresh() re-flattens and re-packs the weights IN PLACE on the current stream (call it after an optimizer step; the module
    must be back in eval mode); after attach_params() the module IS the plain buffer and refresh() only packs.
    The learner's tail on the device: adamw_step(lr) (gradient clipping and AdamW over net.plain from net.grad) and
    sync_from(other) (the target-network update).
    dropout, dropout_seed: what the TRAINING forwards apply (loss_and_grad, forward_batch(training=True)); the module docstring.
    0.0, the default: none, through the entry points and with the bits of a network built without the argument."""

    name, parse = NAME, staticmethod(parse)
    plain_floats, packed_bytes, pack = map(staticmethod, (ops.qnet_plain_floats, ops.qnet_packed_bytes, ops.qnet_pack))

    def __init__(self, model, precision="f32", dropout=0.0, dropout_seed=0):
        self.dropout = dropout_of(parse(model), dropout)           # (attention, dropout1, dropout, dropout2)
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
        q, _ = self._out.get(self._out.rows(boards), _outputs)
        return ops.qnet_forward(boards, self.packed, self.dim_ff, self.n_layers, self.precision, q=q)

    def forward_batch(self, boards, training=False):
        """q float32 (N,4) of the module's own BATCH call on uint8 (N,16) boards, as DQNAgent.train_step makes it
        (hybrid.py:1038-1044): the N boards are one sequence of N tokens that attend to each other, so a row depends on every
        board of the call (g2048_qnet_forward_batch; 2 + 5 n_layers launches, no synchronisation). 1 <= N <= 4096. The weights
        are this network's plain buffer, so refresh() refreshes this path too. f32 only: the first layer's attention logits
        reach 1e9 and bf16 logits would pick keys at random. The output buffer and the workspace are the network's (one of each
        per (N, stream)). training=False: eval mode. training=True: the reference's training-mode call, net.dropout applied with
        the masks of (net.dropout_seed, net.dropout_index); the index then counts on (with dropout 0 too)."""
        if self.precision != "f32":
            raise ValueError("%s.forward_batch: precision 'bf16' is refused: the attention logits reach 1e9 on raw tile values, and "
                             "bf16 logits would pick keys at random; build the network with precision='f32'" % NAME)
        check_batch_layers(self.parsed)
        n = self._out.rows(boards)
        if not training:
            return ops.qnet_forward_batch(boards, self.plain, self.dim_ff, self.n_layers, q=self._out.get(n, _q_only),
                                          workspace=self._out.get(n, self._batch_workspace))
        return ops.qnet_forward_batch(boards, self.plain, self.dim_ff, self.n_layers, q=self._out.get(n, _q_only),
                                      workspace=self._out.get(n, self._batch_workspace), dropout=self.dropout, seed=self.dropout_seed,
                                      call_index=self._next_index())

    def _batch_workspace(self, n, device):          # refuses n = 0 and n above the maximum
        return torch.empty(ops.qnet_batch_workspace_bytes(n, self.dim_ff), dtype=torch.uint8, device=device)

    def _grad_workspace(self, n, device):           # refuses n = 0 and n above the maximum
        return torch.empty(ops.qnet_grad_workspace_bytes(n, self.dim_ff, self.n_layers), dtype=torch.uint8, device=device)

    def _train_workspace(self, n, device):          # loss_and_grad's with dropout: one more array
        return torch.empty(ops.qnet_train_workspace_bytes(n, self.dim_ff, self.n_layers), dtype=torch.uint8, device=device)

    def loss_and_grad(self, boards, actions, targets, weights):
        """(loss float32 (), td_errors float32 (N,), q float32 (N,4)) of DQNAgent.train_step's gradient half (hybrid.py:1038,
        :1049-1055) on uint8 (N,16) boards, int64 (N,) actions, float32 (N,) targets and weights: q = forward_batch(boards) (the
        same bits), td = the Huber error of q[i, actions[i]] against targets[i], loss = mean(weights * td); net.grad is
        OVERWRITTEN with d loss / d parameter in the layout of net.plain (g2048_qnet_loss_grad: the forward with its activations
        kept, then the backward, one phase per launch; no host synchronisation). This is a training forward: net.dropout is
        applied with the masks of (net.dropout_seed, net.dropout_index), regenerated in the backward, and the index counts on;
        with dropout 0 it is g2048_qnet_loss_grad's eval-mode pass, bit for bit. f32 only, for forward_batch's reason. An action outside 0..3 is the caller's error (the kernel reads actions & 3).
        The outputs and the workspace are the network's (one set per (N, stream))."""
        if self.precision != "f32":
            raise ValueError("%s.loss_and_grad: precision 'bf16' is refused: the attention logits reach 1e9 on raw tile values, and "
                             "bf16 logits would pick keys at random; build the network with precision='f32'" % NAME)
        check_batch_layers(self.parsed)
        if not isinstance(boards, torch.Tensor) or boards.dim() != 2:
            raise TypeError("%s.loss_and_grad: boards must be a uint8 (N,16) tensor" % NAME)
        _check_loss_inputs(boards.shape[0], actions, targets, weights)
        n = self._out.rows(boards)
        loss, td, q = self._out.get(n, _loss_outputs)
        ops.qnet_loss_grad(boards, self.plain, actions, targets, weights, self.dim_ff, self.n_layers, grad=self.grad, td=td, loss=loss,
                           q=q, workspace=self._out.get(n, self._train_workspace if any(self.dropout) else self._grad_workspace),
                           dropout=self.dropout, seed=self.dropout_seed, call_index=self._next_index())
        return loss, td, q

    def _step_workspace(self, n, device):
        return torch.empty(ops.qnet_step_workspace_bytes(self.dim_ff, self.n_layers), dtype=torch.uint8, device=device)

    opt_step = 0            # the number of adamw_step calls so far

    def adamw_step(self, lr, max_norm=10.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, step=None):
        """clip_grad_norm_(max_norm) and AdamW.step() of DQNAgent.train_step (hybrid.py:1057-1058) on the device, after
        loss_and_grad: net.plain is updated IN PLACE from net.grad (left clipped, as clip_grad_norm_ leaves it), the moments are
        net.exp_avg and net.exp_avg_sq (g2048_qnet_adamw_step: two launches), then net.packed is packed again, and the module's
        parameters are loaded from net.plain unless attach_params() made them views of it: afterwards the module equals
        net.plain bit for bit either way. Returns the gradient norm before clipping as a float32 () tensor (the network's, one
        per stream), without synchronising. max_norm None: no clipping. lr is this update's learning rate (g2048.cosine_lr).
        step, the update's number in AdamW's bias correction, defaults to net.opt_step + 1; net.opt_step counts the CALLS: a
        gradient with an inf or a NaN leaves weights, gradient and moments untouched (the returned norm is then not finite),
        and that skipped call still counts, because the host never learns of it. f32 only. The LayerNorm-eps slots are
        settings and are not updated."""
        if self.precision != "f32":
            raise ValueError("%s.adamw_step: precision 'bf16' is refused: loss_and_grad is f32 only; build the network with "
                             "precision='f32'" % NAME)
        step = self.opt_step + 1 if step is None else int(step)
        norm = ops.qnet_adamw_step(self.plain, self.grad, self.exp_avg, self.exp_avg_sq, self.dim_ff, self.n_layers, lr, step, betas=betas,
                                   eps=eps, weight_decay=weight_decay, max_norm=max_norm, norm=self._out.get(0, _norm_out),
                                   workspace=self._out.get(0, self._step_workspace))
        self.opt_step += 1
        self._plain_changed()
        return norm

    def sync_from(self, other):
        """The target-network update (DQNAgent.update_target_model, hybrid.py:811, :1073) without a state_dict round: ONE device
        copy of other.plain into net.plain, net.packed packed again at this network's own precision, and the module's
        parameters loaded from net.plain unless attach_params() made them views of it. Weights only: dropout, dropout_seed and
        dropout_index stay this network's own. The two networks of a learner are built with different seeds, e.g.
        DeviceQNetwork(online_model, dropout=p, dropout_seed=s) and DeviceQNetwork(target_model, dropout=p, dropout_seed=s + 1);
        with the same seed and index their masks coincide. Raises ValueError when dim_ff,
        n_layers, the LayerNorm eps or the device differ."""
        if not isinstance(other, DeviceQNetwork):
            raise TypeError("%s.sync_from: expected a %s, got %s" % (NAME, NAME, type(other).__name__))
        if (other.dim_ff, other.n_layers) != (self.dim_ff, self.n_layers):
            raise ValueError("%s.sync_from: the other network has dim_ff %d and %d layers, this one dim_ff %d and %d layers"
                             % (NAME, other.dim_ff, other.n_layers, self.dim_ff, self.n_layers))
        if other.device != self.device:
            raise ValueError("%s.sync_from: the other network is on %s, this one on %s" % (NAME, other.device, self.device))
        mine, theirs = ([t for t in n.parsed.plain_tensors() if not isinstance(t, torch.Tensor)] for n in (self, other))
        if mine != theirs:
            raise ValueError("%s.sync_from: the two modules' LayerNorm eps differ (%s, %s): they are settings, not weights" % (NAME, theirs, mine))
        self.plain.copy_(other.plain)
        self._plain_changed()
        return self

    def act(self, boards, epsilon=0.0, seed=0x2048, step_index=0, id_base=0):
        """(actions, q). epsilon > 0 adds one g2048_qnet_select_actions launch: DQNAgent.select_action's epsilon-greedy with the
        reference's biased exploration (use_beam_search = False), the draws keyed by (seed, step_index, id_base + row)."""
        n = self._out.rows(boards)
        q, actions = self._out.get(n, _outputs)
        ops.qnet_forward(boards, self.packed, self.dim_ff, self.n_layers, self.precision, q=q, actions=actions)
        if epsilon > 0:
            ops.qnet_select_actions(q, boards, epsilon, seed, step_index, id_base, actions=actions, explored=self._out.get(n, _explored))
        return actions, q

    def act_beam(self, boards, epsilon=0.0, seed=0x2048, step_index=0, id_base=0, beam_width=15, search_depth=30,
                 beam_search_threshold=64, gamma=0.99):
        """(actions, q): act with the reference's use_beam_search = True (DQNAgent.select_action, hybrid.py:909-953; the defaults
        are DQNAgent's own settings). Where beam_search plans -- max tile >= beam_search_threshold and at least 8 tiles -- the
        exploit action is its decision, elsewhere the argmax of q; at the reference's settings the network therefore decides only
        boards below 64 or with fewer than 8 tiles. search_depth >= 2: the forward plus ONE g2048_qnet_beam_actions launch (the
        search consults no network and no draw). search_depth 1: forward, g2048_qnet_beam_expand (draws keyed by (seed, SIMULATE,
        step_index, id_base + row)), the forward on the n x 32 candidate boards, then the decision."""
        n = self._out.rows(boards)
        q, actions = self._out.get(n, _outputs)
        ops.qnet_forward(boards, self.packed, self.dim_ff, self.n_layers, self.precision, q=q)
        succ_q = None
        if int(search_depth) == 1:
            succ, count, succ_q = self._out.get(n, _candidates)
            ops.qnet_beam_expand(boards, seed, step_index, id_base, succ=succ, count=count)
            ops.qnet_forward(succ.view(n * 32, 16), self.packed, self.dim_ff, self.n_layers, self.precision, q=succ_q)
            succ_q = succ_q.view(n, 32, 4)
        ops.qnet_beam_actions(q, boards, succ_q, beam_width, search_depth, beam_search_threshold, gamma, epsilon, seed, step_index,
                              id_base, actions=actions, planned=self._out.get(n, _planned), explored=self._out.get(n, _explored))
        return actions, q


def dqn_targets(online, target, next_boards, shaped_rewards, dones, gamma=0.99, training=False):
    """The no-gradient block of DQNAgent.train_step (agents/hybrid.py:1041-1046) on the device: (targets float32 (N,),
    next_actions int64 (N,)) with next_actions = online.forward_batch(next_boards).argmax(1) (unmasked, first maximum), next_q
    = target.forward_batch(next_boards) at those actions and targets = shaped_rewards + (1 - dones) * gamma * next_q. online,
    target: DeviceQNetwork; next_boards uint8 (N,16); shaped_rewards, dones float32 (N,) as DeviceReplayBuffer.sample returns
    them. Three launch groups on the current stream, no host synchronisation; the outputs are buffers of `online` (one pair per
    (N, stream)). training=True: both forwards are training forwards, as the reference's are (neither module is ever put in eval
    mode): each network applies its own dropout with its own seed and index."""
    q_online = online.forward_batch(next_boards, training=training)
    q_target = target.forward_batch(next_boards, training=training)
    targets, next_actions = online._out.get(next_boards.shape[0], _targets)
    return ops.dqn_targets(q_online, q_target, shaped_rewards, dones, gamma, targets=targets, next_actions=next_actions)


def cosine_lr(t, base_lr=1e-3, t_max=150000, eta_min=1e-4):
    """The learning rate of torch's CosineAnnealingLR(T_max=t_max, eta_min=eta_min) over an optimizer of lr base_lr after t
    scheduler.step() calls, 0 <= t <= t_max, in closed form (the defaults are DQNAgent's: hybrid.py:782-783). Pure Python."""
    import math
    if not 0 <= t <= t_max:
        raise ValueError("g2048: cosine_lr is defined for 0 <= t <= t_max (got t = %s, t_max = %s)" % (t, t_max))
    return eta_min + (base_lr - eta_min) * (1.0 + math.cos(math.pi * t / t_max)) / 2.0


def dqn_epsilon(step_counter, start=1.0, end=0.001, decay_steps=150000):
    """DQNAgent's exploration rate after step_counter train_step calls (hybrid.py:1068-1070): progress = min(step_counter /
    decay_steps, 1), epsilon = max(end, start - (start - end) * progress ** 0.6). Pure Python."""
    progress = min(step_counter / decay_steps, 1.0)
    return max(end, start - (start - end) * (progress ** 0.6))
