"""The hybrid agent's CNN-transformer Q-network (agents/hybrid.py:700-727, HybridDQN, eval mode) as one HIP launch on the
packed boards.

`DeviceQNetwork(model, precision="f32")` takes a torch module of that structure, flattens its parameters into the plain layout
of include/g2048.h (state-dict order, plus the two LayerNorm eps per layer), packs them with `g2048_qnet_pack` and runs
`g2048_qnet_forward` on uint8 (N,16) boards.

Per-board semantics. The reference's encoder layer is not batch_first and is fed x.unsqueeze(1), so model(x) on a batch of B
boards is ONE sequence of B tokens that attend to each other; the reference only ever calls it with one board. Row i here is
model(x[i:i+1]): every board is a sequence of one token, the attention softmax is exactly 1.0 and the attention block is
out_proj(W_v x + b_v). Q, K, the head count and batch_first cannot influence that and are not constrained. The reference never
calls .eval() (its dropout is live even in select_action); this is the eval-mode function.

The module is recognised by structure, not by attribute names: two Conv2d (1->32 and 32->64, kernel 2, stride 1, paddings 1 and
0), exactly one nn.TransformerEncoder (post-norm ReLU layers, d_model 128, no final norm, dim_feedforward a multiple of 32) and,
outside it, two Linears told apart by shape: 1024->128 (embedding) and 128->4 (fc). ReLU / Sequential containers around them are
ignored. Anything else raises ValueError with the reason; a module in training mode is refused (dropout has no device
counterpart).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops

D_MODEL = 128
_ROLES = {(1024, 128): "embedding", (128, 4): "fc"}
_CONVS = {(1, 32): ("conv1", 1), (32, 64): ("conv2", 0)}           # (in, out) channels: role, padding


class Parsed:
    """The module's parts: conv1, conv2, embedding, layers (TransformerEncoderLayer list), fc, dim_ff."""
    __slots__ = ("conv1", "conv2", "embedding", "layers", "fc", "dim_ff")


def _refuse(msg):
    raise ValueError("DeviceQNetwork: " + msg)


def _check_layer(i, lay, dim_ff):
    where = "encoder layer %d" % i
    if not isinstance(lay, nn.TransformerEncoderLayer):
        _refuse("%s is a %s, not an nn.TransformerEncoderLayer" % (where, type(lay).__name__))
    if lay.norm_first:
        _refuse("%s has norm_first=True (only post-norm layers are supported)" % where)
    act = lay.activation
    if not (act is F.relu or act is torch.relu or isinstance(act, nn.ReLU)):
        _refuse("%s has an activation other than ReLU" % where)
    att = lay.self_attn
    if att.embed_dim != D_MODEL:
        _refuse("%s has d_model %d, expected %d" % (where, att.embed_dim, D_MODEL))
    if att.in_proj_weight is None or att.bias_k is not None or att.add_zero_attn:
        _refuse("%s has an attention variant other than the plain packed q/k/v projection" % where)
    if lay.linear1.out_features % 32 != 0:
        _refuse("%s has dim_ff %d, not a multiple of 32" % (where, lay.linear1.out_features))
    if lay.linear1.out_features != dim_ff:
        _refuse("%s has dim_ff %d, layer 0 has %d" % (where, lay.linear1.out_features, dim_ff))
    if att.in_proj_bias is None or att.out_proj.bias is None or lay.linear1.bias is None or lay.linear2.bias is None:
        _refuse("%s has a projection with a missing bias" % where)
    for norm in (lay.norm1, lay.norm2):
        if not isinstance(norm, nn.LayerNorm) or norm.weight is None or norm.bias is None:
            _refuse("%s needs LayerNorms with weight and bias" % where)


def _conv_role(m):
    what = "Conv2d %d->%d" % (m.in_channels, m.out_channels)
    role = _CONVS.get((m.in_channels, m.out_channels))
    if role is None:
        _refuse("unexpected %s" % what)
    name, pad = role
    if tuple(m.kernel_size) != (2, 2) or tuple(m.stride) != (1, 1):
        _refuse("the %s needs kernel 2 and stride 1 (got kernel %s, stride %s)" % (what, tuple(m.kernel_size), tuple(m.stride)))
    if m.padding != (pad, pad) or m.padding_mode != "zeros":
        _refuse("the %s needs zero padding %d (got %s, %s)" % (what, pad, m.padding, m.padding_mode))
    if tuple(m.dilation) != (1, 1) or m.groups != 1:
        _refuse("the %s has dilation or groups other than 1" % what)
    if m.bias is None:
        _refuse("the %s has a missing bias" % what)
    return name


def parse(module):
    """The module as a Parsed record. Raises ValueError naming the reason."""
    if not isinstance(module, nn.Module):
        _refuse("expected a torch.nn.Module, got %s" % type(module).__name__)
    if any(m.training for m in module.modules()):
        _refuse("%s is in training mode; call .eval() first (inference only)" % type(module).__name__)
    encoders = [m for m in module.modules() if isinstance(m, nn.TransformerEncoder)]
    if len(encoders) != 1:
        _refuse("expected exactly one nn.TransformerEncoder, found %d" % len(encoders))
    enc = encoders[0]
    if enc.norm is not None:
        _refuse("the encoder has a final norm (encoder.norm), which the reference's model does not")
    if len(enc.layers) < 1:
        _refuse("the encoder has no layers")
    inside = set(id(m) for m in enc.modules())
    out = Parsed()
    found = {}
    for m in module.modules():
        if id(m) in inside:
            continue
        if isinstance(m, nn.Conv2d):
            role = _conv_role(m)
            if role in found:
                _refuse("duplicate Conv2d %d->%d" % (m.in_channels, m.out_channels))
            found[role] = m
        elif isinstance(m, nn.Linear):
            role = _ROLES.get((m.in_features, m.out_features))
            if role is None:
                _refuse("unexpected Linear %d->%d outside the encoder" % (m.in_features, m.out_features))
            if role in found:
                _refuse("duplicate Linear %d->%d (%s)" % (m.in_features, m.out_features, role))
            if m.bias is None:
                _refuse("the %s Linear %d->%d has a missing bias" % (role, m.in_features, m.out_features))
            found[role] = m
    for (i, o), (role, _) in _CONVS.items():
        if role not in found:
            _refuse("missing Conv2d %d->%d (%s)" % (i, o, role))
    for (i, o), role in _ROLES.items():
        if role not in found:
            _refuse("missing Linear %d->%d (%s)" % (i, o, role))
    for role, m in found.items():
        setattr(out, role, m)
    out.layers = list(enc.layers)
    first = out.layers[0]
    out.dim_ff = first.linear1.out_features if isinstance(first, nn.TransformerEncoderLayer) else 0
    for i, lay in enumerate(out.layers):
        _check_layer(i, lay, out.dim_ff)
    return out


def plain_tensors(p):
    """The parameters in the order of g2048_qnet_pack's plain layout (LayerNorm eps as Python floats)."""
    seq = [p.conv1.weight, p.conv1.bias, p.conv2.weight, p.conv2.bias, p.embedding.weight, p.embedding.bias]
    for lay in p.layers:
        a = lay.self_attn
        seq += [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, lay.linear1.weight, lay.linear1.bias,
                lay.linear2.weight, lay.linear2.bias, lay.norm1.weight, lay.norm1.bias, lay.norm2.weight, lay.norm2.bias,
                float(lay.norm1.eps), float(lay.norm2.eps)]
    seq += [p.fc.weight, p.fc.bias]
    return seq


@torch.no_grad()
def flatten(p, out=None):
    """The plain float32 buffer of a Parsed module (on the module's device; written in place when `out` is given)."""
    seq = plain_tensors(p)
    total = sum(t.numel() if isinstance(t, torch.Tensor) else 1 for t in seq)
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=p.embedding.weight.device)
    if out.numel() != total:
        raise ValueError("DeviceQNetwork: the plain buffer holds %d floats, the module has %d" % (out.numel(), total))
    o = 0
    for t in seq:
        if isinstance(t, torch.Tensor):
            out[o:o + t.numel()].copy_(t.reshape(-1))
            o += t.numel()
        else:
            out[o:o + 1].fill_(t)
            o += 1
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
    def w(t):
        t = t.detach()
        if round_weights is not None:
            t = round_weights(t)
        return t.to(dtype)
    x = tile_values(boards, dtype).reshape(-1, 1, 4, 4)
    x = torch.relu(F.conv2d(x, w(p.conv1.weight), w(p.conv1.bias), padding=1))
    x = torch.relu(F.conv2d(x, w(p.conv2.weight), w(p.conv2.bias)))
    x = x.reshape(x.shape[0], -1) @ w(p.embedding.weight).T + w(p.embedding.bias)
    for lay in p.layers:
        a = lay.self_attn
        v = x @ w(a.in_proj_weight)[2 * D_MODEL:].T + w(a.in_proj_bias)[2 * D_MODEL:]
        x = F.layer_norm(x + v @ w(a.out_proj.weight).T + w(a.out_proj.bias), (D_MODEL,), w(lay.norm1.weight), w(lay.norm1.bias), lay.norm1.eps)
        h = torch.relu(x @ w(lay.linear1.weight).T + w(lay.linear1.bias))
        x = F.layer_norm(x + h @ w(lay.linear2.weight).T + w(lay.linear2.bias), (D_MODEL,), w(lay.norm2.weight), w(lay.norm2.bias), lay.norm2.eps)
    return x @ w(p.fc.weight).T + w(p.fc.bias)


class DeviceQNetwork:
    """Hybrid Q-network on the device: __call__(boards uint8 (N,16)) -> q float32 (N,4); act(boards) -> (actions uint8 (N,), q),
    the exploit action of DQNAgent.select_action (argmax of q over the env's valid moves, ties to the lowest index, 0 for a board
    with no valid move); act(boards, epsilon, seed, step_index, id_base) with epsilon > 0 is the whole epsilon-greedy
    select_action (one more launch). One g2048_qnet_forward launch per call; the outputs are buffers owned by the network (one set per
    (N, stream), overwritten by the next call with the same N on the same stream), so after the first call per (N, stream) a
    call neither allocates nor synchronises.

    precision: "f32" (exact f32 MFMA, the parity path) or "bf16" (bf16 weights and matmul inputs, f32 accumulation, biases,
    LayerNorm and residual adds).
    refresh() re-flattens and re-packs the weights IN PLACE on the current stream (call it after an optimizer step; the module
    must be back in eval mode)."""

    def __init__(self, model, precision="f32"):
        if precision not in ops.POLICY_PRECISIONS:
            raise ValueError("DeviceQNetwork: precision must be 'f32' or 'bf16'")
        self.model, self.precision = model, precision
        self.parsed = parse(model)
        self.dim_ff, self.n_layers = self.parsed.dim_ff, len(self.parsed.layers)
        self.device = self.parsed.embedding.weight.device
        if self.device.type != "cuda":
            raise RuntimeError("g2048: DeviceQNetwork needs the module on a ROCm device (got %s); there is no CPU path" % self.device)
        self.plain = torch.empty(ops.qnet_plain_floats(self.dim_ff, self.n_layers), dtype=torch.float32, device=self.device)
        self.packed = torch.empty(ops.qnet_packed_bytes(precision, self.dim_ff, self.n_layers), dtype=torch.uint8, device=self.device)
        self._out, self._explored = {}, {}
        self.refresh()

    def refresh(self):
        if any(m.training for m in self.model.modules()):
            raise ValueError("DeviceQNetwork.refresh: %s is in training mode; call .eval() first" % type(self.model).__name__)
        flatten(self.parsed, self.plain)
        ops.qnet_pack(self.plain, self.dim_ff, self.n_layers, self.precision, out=self.packed)

    def _buffers(self, boards):
        L.require_device_tensor(boards, torch.uint8, (16,), "boards")
        if boards.device != self.device:
            raise ValueError("DeviceQNetwork: boards on %s, weights on %s" % (boards.device, self.device))
        n = boards.shape[0]
        key = (n, torch.cuda.current_stream(self.device).cuda_stream)
        bufs = self._out.get(key)
        if bufs is None:
            bufs = (torch.empty((n, 4), dtype=torch.float32, device=self.device), torch.empty(n, dtype=torch.uint8, device=self.device))
            self._out[key] = bufs
        return bufs

    def __call__(self, boards):
        q, _ = self._buffers(boards)
        return ops.qnet_forward(boards, self.packed, self.dim_ff, self.n_layers, self.precision, q=q)

    def act(self, boards, epsilon=0.0, seed=0x2048, step_index=0, id_base=0):
        """(actions, q). epsilon > 0 adds one g2048_qnet_select_actions launch: DQNAgent.select_action's epsilon-greedy with the
        reference's biased exploration (use_beam_search = False), the draws keyed by (seed, step_index, id_base + row)."""
        q, actions = self._buffers(boards)
        ops.qnet_forward(boards, self.packed, self.dim_ff, self.n_layers, self.precision, q=q, actions=actions)
        if epsilon > 0:
            key = (boards.shape[0], torch.cuda.current_stream(self.device).cuda_stream)
            explored = self._explored.get(key)
            if explored is None:
                explored = self._explored[key] = torch.empty(boards.shape[0], dtype=torch.uint8, device=self.device)
            ops.qnet_select_actions(q, boards, epsilon, seed, step_index, id_base, actions=actions, explored=explored)
        return actions, q
