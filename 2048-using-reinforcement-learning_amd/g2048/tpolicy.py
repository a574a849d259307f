"""The reference's transformer policy (models/transformer.py:4-40, eval mode) as one HIP launch on the packed boards.

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
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops

D_MODEL, N_HEAD, TOKENS = 64, 4, 16
_ROLES = {(1, 64): "embedding", (1024, 128): "fc1", (128, 64): "fc2", (64, 4): "actor", (64, 1): "critic"}


class Parsed:
    """The module's parts: embedding, layers (TransformerEncoderLayer list), fc1, fc2, actor, critic, dim_ff."""
    __slots__ = ("embedding", "layers", "fc1", "fc2", "actor", "critic", "dim_ff")


def _refuse(msg):
    raise ValueError("DeviceTransformerPolicy: " + msg)


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
    if not att.batch_first:
        _refuse("%s has batch_first=False" % where)
    if att.embed_dim != D_MODEL:
        _refuse("%s has d_model %d, expected %d" % (where, att.embed_dim, D_MODEL))
    if att.num_heads != N_HEAD:
        _refuse("%s has nhead %d, expected %d" % (where, att.num_heads, N_HEAD))
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
        if not isinstance(m, nn.Linear) or id(m) in inside:
            continue
        role = _ROLES.get((m.in_features, m.out_features))
        if role is None:
            _refuse("unexpected Linear %d->%d outside the encoder" % (m.in_features, m.out_features))
        if role in found:
            _refuse("duplicate Linear %d->%d (%s)" % (m.in_features, m.out_features, role))
        if m.bias is None:
            _refuse("the %s Linear %d->%d has a missing bias" % (role, m.in_features, m.out_features))
        found[role] = m
    for (i, o), role in _ROLES.items():
        if role not in found:
            _refuse("missing Linear %d->%d (%s)" % (i, o, role))
        setattr(out, role, found[role])
    out.layers = list(enc.layers)
    first = out.layers[0]
    out.dim_ff = first.linear1.out_features if isinstance(first, nn.TransformerEncoderLayer) else 0
    for i, lay in enumerate(out.layers):
        _check_layer(i, lay, out.dim_ff)
    return out


def plain_tensors(p):
    """The parameters in the order of g2048_tpolicy_pack's plain layout (LayerNorm eps as Python floats)."""
    seq = [p.embedding.weight, p.embedding.bias]
    for lay in p.layers:
        a = lay.self_attn
        seq += [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, lay.linear1.weight, lay.linear1.bias,
                lay.linear2.weight, lay.linear2.bias, lay.norm1.weight, lay.norm1.bias, lay.norm2.weight, lay.norm2.bias,
                float(lay.norm1.eps), float(lay.norm2.eps)]
    seq += [p.fc1.weight, p.fc1.bias, p.fc2.weight, p.fc2.bias, p.actor.weight, p.actor.bias, p.critic.weight, p.critic.bias]
    return seq


@torch.no_grad()
def flatten(p, out=None):
    """The plain float32 buffer of a Parsed module (on the module's device; written in place when `out` is given)."""
    seq = plain_tensors(p)
    total = sum(t.numel() if isinstance(t, torch.Tensor) else 1 for t in seq)
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=p.embedding.weight.device)
    if out.numel() != total:
        raise ValueError("DeviceTransformerPolicy: the plain buffer holds %d floats, the module has %d" % (out.numel(), total))
    o = 0
    for t in seq:
        if isinstance(t, torch.Tensor):
            out[o:o + t.numel()].copy_(t.reshape(-1))
            o += t.numel()
        else:
            out[o:o + 1].fill_(t)
            o += 1
    return out


@torch.no_grad()
def unflatten(p, plain):
    """Loads a plain buffer back into the Parsed module's parameters (the inverse of flatten; eps entries are skipped)."""
    o = 0
    for t in plain_tensors(p):
        if isinstance(t, torch.Tensor):
            t.copy_(plain[o:o + t.numel()].reshape(t.shape))
            o += t.numel()
        else:
            o += 1
    return p


@torch.no_grad()
def forward_reference(p, boards, dtype=torch.float64, round_weights=None):
    """The parsed network on uint8 (N,16) boards with plain torch ops in `dtype` (any device): the yardstick of the kernel.
    round_weights: an optional function applied to every parameter first (e.g. a bf16 round trip)."""
    def w(t):
        t = t.detach()
        if round_weights is not None:
            t = round_weights(t)
        return t.to(dtype)
    x = boards.to(dtype) / 15
    x = x.reshape(-1, TOKENS, 1) * w(p.embedding.weight).reshape(1, 1, -1) + w(p.embedding.bias)
    n = x.shape[0]
    for lay in p.layers:
        a = lay.self_attn
        qkv = x @ w(a.in_proj_weight).T + w(a.in_proj_bias)
        q, k, v = (t.reshape(n, TOKENS, N_HEAD, -1).transpose(1, 2) for t in qkv.split(D_MODEL, -1))
        s = torch.softmax((q @ k.transpose(-1, -2)) / 4, -1)
        o = (s @ v).transpose(1, 2).reshape(n, TOKENS, D_MODEL)
        x = F.layer_norm(x + o @ w(a.out_proj.weight).T + w(a.out_proj.bias), (D_MODEL,), w(lay.norm1.weight), w(lay.norm1.bias), lay.norm1.eps)
        h = torch.relu(x @ w(lay.linear1.weight).T + w(lay.linear1.bias))
        x = F.layer_norm(x + h @ w(lay.linear2.weight).T + w(lay.linear2.bias), (D_MODEL,), w(lay.norm2.weight), w(lay.norm2.bias), lay.norm2.eps)
    h = torch.relu(x.reshape(n, -1) @ w(p.fc1.weight).T + w(p.fc1.bias))
    h = torch.relu(h @ w(p.fc2.weight).T + w(p.fc2.bias))
    return torch.softmax(h @ w(p.actor.weight).T + w(p.actor.bias), -1), h @ w(p.critic.weight).T + w(p.critic.bias)


class DeviceTransformerPolicy:
    """Transformer policy on the device: __call__(boards uint8 (N,16)) -> (probs float32 (N,4), value float32 (N,1)). One
    g2048_tpolicy_forward launch per call; the outputs are buffers owned by the policy (one pair per (N, stream), overwritten
    by the next call with the same N on the same stream), so after the first call per (N, stream) a call neither allocates nor
    synchronises and can be captured in a graph (RolloutCollector does).

    precision: "f32" (exact f32 MFMA, the parity path) or "bf16" (bf16 weights and matmul inputs, f32 accumulation, LayerNorm,
    softmax and attention products).
    refresh() re-flattens and re-packs the weights IN PLACE on the current stream (call it after an optimizer step; the module
    must be back in eval mode): graphs captured earlier replay with the new weights.

    takes_boards = True: RolloutCollector hands it the packed boards instead of the float observations."""

    takes_boards = True

    def __init__(self, model, precision="f32"):
        if precision not in ops.POLICY_PRECISIONS:
            raise ValueError("DeviceTransformerPolicy: precision must be 'f32' or 'bf16'")
        self.model, self.precision = model, precision
        self.parsed = parse(model)
        self.dim_ff, self.n_layers = self.parsed.dim_ff, len(self.parsed.layers)
        self.device = self.parsed.embedding.weight.device
        if self.device.type != "cuda":
            raise RuntimeError("g2048: DeviceTransformerPolicy needs the module on a ROCm device (got %s); there is no CPU path" % self.device)
        self.plain = torch.empty(ops.tpolicy_plain_floats(self.dim_ff, self.n_layers), dtype=torch.float32, device=self.device)
        self.packed = torch.empty(ops.tpolicy_packed_bytes(precision, self.dim_ff, self.n_layers), dtype=torch.uint8, device=self.device)
        self._out = {}
        self.refresh()

    def refresh(self):
        if any(m.training for m in self.model.modules()):
            raise ValueError("DeviceTransformerPolicy.refresh: %s is in training mode; call .eval() first" % type(self.model).__name__)
        flatten(self.parsed, self.plain)
        ops.tpolicy_pack(self.plain, self.dim_ff, self.n_layers, self.precision, out=self.packed)

    def __call__(self, boards):
        L.require_device_tensor(boards, torch.uint8, (16,), "boards")
        if boards.device != self.device:
            raise ValueError("DeviceTransformerPolicy: boards on %s, weights on %s" % (boards.device, self.device))
        n = boards.shape[0]
        key = (n, torch.cuda.current_stream(self.device).cuda_stream)
        bufs = self._out.get(key)
        if bufs is None:
            bufs = (torch.empty((n, 4), dtype=torch.float32, device=self.device), torch.empty((n, 1), dtype=torch.float32, device=self.device))
            self._out[key] = bufs
        return ops.tpolicy_forward(boards, self.packed, self.dim_ff, self.n_layers, self.precision, probs=bufs[0], value=bufs[1])
