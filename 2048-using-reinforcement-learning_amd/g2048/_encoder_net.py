"""What the networks built around an nn.TransformerEncoder (tpolicy.py, qnet.py) share on the host: recognising the module by
structure, the plain parameter layout of an encoder layer, flatten / unflatten over a network's plain layout, the pieces of the
float64 yardsticks, and the device-side wrapper (constructor, refresh(), boards check, output buffers). A refusal is a ValueError
whose text starts with the network's display name.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops


def _refuse(name, msg):
    raise ValueError(name + ": " + msg)


def find_encoder(name, module):
    """The one nn.TransformerEncoder of an eval-mode module (no final norm, at least one layer)."""
    if not isinstance(module, nn.Module):
        _refuse(name, "expected a torch.nn.Module, got %s" % type(module).__name__)
    if any(m.training for m in module.modules()):
        _refuse(name, "%s is in training mode; call .eval() first (inference only)" % type(module).__name__)
    encoders = [m for m in module.modules() if isinstance(m, nn.TransformerEncoder)]
    if len(encoders) != 1:
        _refuse(name, "expected exactly one nn.TransformerEncoder, found %d" % len(encoders))
    enc = encoders[0]
    if enc.norm is not None:
        _refuse(name, "the encoder has a final norm (encoder.norm), which the reference's model does not")
    if len(enc.layers) < 1:
        _refuse(name, "the encoder has no layers")
    return enc


def claim_by_shape(name, module, enc, out, linears, convs=None, check_conv=None):
    """Sets out.<role> to the module's Linears outside the encoder, told apart by (in, out) features: linears = {shape: role}.
    convs: the same for its Conv2ds by (in, out) channels, each passed to check_conv(m, role, what) when it is met."""
    inside = set(id(m) for m in enc.modules())
    found = {}
    for m in module.modules():
        if id(m) in inside:
            continue
        if convs is not None and isinstance(m, nn.Conv2d):
            what = "Conv2d %d->%d" % (m.in_channels, m.out_channels)
            role = convs.get((m.in_channels, m.out_channels))
            if role is None:
                _refuse(name, "unexpected %s" % what)
            check_conv(m, role, what)
            if role in found:
                _refuse(name, "duplicate %s" % what)
        elif isinstance(m, nn.Linear):
            what = "Linear %d->%d" % (m.in_features, m.out_features)
            role = linears.get((m.in_features, m.out_features))
            if role is None:
                _refuse(name, "unexpected %s outside the encoder" % what)
            if role in found:
                _refuse(name, "duplicate %s (%s)" % (what, role))
            if m.bias is None:
                _refuse(name, "the %s %s has a missing bias" % (role, what))
        else:
            continue
        found[role] = m
    for kind, roles in (("Conv2d", convs or {}), ("Linear", linears)):
        for (i, o), role in roles.items():
            if role not in found:
                _refuse(name, "missing %s %d->%d (%s)" % (kind, i, o, role))
    for role, m in found.items():
        setattr(out, role, m)


def _check_layer(name, i, lay, dim_ff, d_model, nhead, batch_first):
    where = "encoder layer %d" % i
    if not isinstance(lay, nn.TransformerEncoderLayer):
        _refuse(name, "%s is a %s, not an nn.TransformerEncoderLayer" % (where, type(lay).__name__))
    if lay.norm_first:
        _refuse(name, "%s has norm_first=True (only post-norm layers are supported)" % where)
    act = lay.activation
    if not (act is F.relu or act is torch.relu or isinstance(act, nn.ReLU)):
        _refuse(name, "%s has an activation other than ReLU" % where)
    att = lay.self_attn
    if batch_first and not att.batch_first:
        _refuse(name, "%s has batch_first=False" % where)
    if att.embed_dim != d_model:
        _refuse(name, "%s has d_model %d, expected %d" % (where, att.embed_dim, d_model))
    if nhead is not None and att.num_heads != nhead:
        _refuse(name, "%s has nhead %d, expected %d" % (where, att.num_heads, nhead))
    if att.in_proj_weight is None or att.bias_k is not None or att.add_zero_attn:
        _refuse(name, "%s has an attention variant other than the plain packed q/k/v projection" % where)
    if lay.linear1.out_features % 32 != 0:
        _refuse(name, "%s has dim_ff %d, not a multiple of 32" % (where, lay.linear1.out_features))
    if lay.linear1.out_features != dim_ff:
        _refuse(name, "%s has dim_ff %d, layer 0 has %d" % (where, lay.linear1.out_features, dim_ff))
    if att.in_proj_bias is None or att.out_proj.bias is None or lay.linear1.bias is None or lay.linear2.bias is None:
        _refuse(name, "%s has a projection with a missing bias" % where)
    for norm in (lay.norm1, lay.norm2):
        if not isinstance(norm, nn.LayerNorm) or norm.weight is None or norm.bias is None:
            _refuse(name, "%s needs LayerNorms with weight and bias" % where)


def checked_layers(name, enc, d_model, nhead=None, batch_first=False):
    """(layers, dim_ff) of the encoder: post-norm ReLU layers of d_model, all of layer 0's dim_feedforward (a multiple of 32).
    nhead / batch_first: constraints only a network whose tokens attend to each other has."""
    layers = list(enc.layers)
    first = layers[0]
    dim_ff = first.linear1.out_features if isinstance(first, nn.TransformerEncoderLayer) else 0
    for i, lay in enumerate(layers):
        _check_layer(name, i, lay, dim_ff, d_model, nhead, batch_first)
    return layers, dim_ff


def dropout_of(name, p, dropout):
    """The four dropout probabilities (attention, dropout1, dropout, dropout2) of a device network's `dropout` argument for the
    parsed module p: a probability for all four sites, a 4-tuple, or "module" for the layers' own self_attn.dropout, dropout1.p,
    dropout.p and dropout2.p, which must agree from layer to layer (the masks differ per layer, the probabilities are shared).
    Raises ValueError for anything else and for a probability outside 0 <= p < 1."""
    if isinstance(dropout, str):
        if dropout != "module":
            _refuse(name, "dropout must be a probability, a 4-tuple %s or \"module\", got %r" % (ops.QNET_DROPOUT_SITES, dropout))
        per_layer = [(float(lay.self_attn.dropout), float(lay.dropout1.p), float(lay.dropout.p), float(lay.dropout2.p)) for lay in p.layers]
        for i, t in enumerate(per_layer):
            if t != per_layer[0]:
                _refuse(name, "dropout=\"module\": encoder layer %d has dropout %s, layer 0 has %s; the device pass shares one set of "
                              "probabilities among the layers" % (i, t, per_layer[0]))
        dropout = per_layer[0]
    try:
        return ops.qnet_dropout_p(dropout) or (0.0, 0.0, 0.0, 0.0)
    except (TypeError, ValueError) as e:
        _refuse(name, str(e)[7:] if str(e).startswith("g2048: ") else "dropout: " + str(e))


def layer_tensors(layers):
    """The encoder layers' parameters in the plain layout's order: state-dict order, then the two LayerNorm eps as Python floats."""
    seq = []
    for lay in layers:
        a = lay.self_attn
        seq += [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, lay.linear1.weight, lay.linear1.bias,
                lay.linear2.weight, lay.linear2.bias, lay.norm1.weight, lay.norm1.bias, lay.norm2.weight, lay.norm2.bias,
                float(lay.norm1.eps), float(lay.norm2.eps)]
    return seq


@torch.no_grad()
def flatten(p, out=None):
    """The plain float32 buffer of a Parsed module (on the module's device; written in place when `out` is given). A Parsed
    record has its network's display name as `name` and its plain layout as plain_tensors()."""
    seq = p.plain_tensors()
    total = sum(t.numel() if isinstance(t, torch.Tensor) else 1 for t in seq)
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=p.embedding.weight.device)
    if out.numel() != total:
        raise ValueError("%s: the plain buffer holds %d floats, the module has %d" % (p.name, out.numel(), total))
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
    for t in p.plain_tensors():
        if isinstance(t, torch.Tensor):
            t.copy_(plain[o:o + t.numel()].reshape(t.shape))
            o += t.numel()
        else:
            o += 1
    return p


def weight_caster(dtype, round_weights=None):
    """w(parameter) of a forward_reference: detached, through round_weights if given (e.g. a bf16 round trip), then in dtype."""
    def w(t):
        t = t.detach()
        if round_weights is not None:
            t = round_weights(t)
        return t.to(dtype)
    return w


def post_norm_tail(lay, x, attended, w, mult=None, feed_forward=None):
    """The rest of a post-norm encoder layer after the attention itself: norm1(x + out_proj(attended)), then the feed-forward
    pair and norm2, with the weights through w. mult: None (eval mode), or a callable (site, shape, dtype) -> the multipliers of
    dropout site 1 (dropout1), 2 (the hidden layer's) or 3 (dropout2) of this layer, applied where the training-mode layer drops.
    feed_forward: None, or a callable (x, W1, b1, W2, b2, m2) -> linear2(m2(relu(linear1(x)))) that takes the place of the two plain
    products (m2 applies the site-2 multipliers): the bf16 restatement of g2048.tpolicy."""
    a, d = lay.self_attn, (x.shape[-1],)
    m = (lambda site, t: t) if mult is None else (lambda site, t: t * mult(site, tuple(t.shape), t.dtype))
    x = F.layer_norm(x + m(1, attended @ w(a.out_proj.weight).T + w(a.out_proj.bias)), d, w(lay.norm1.weight), w(lay.norm1.bias), lay.norm1.eps)
    if feed_forward is not None:
        y = feed_forward(x, w(lay.linear1.weight), w(lay.linear1.bias), w(lay.linear2.weight), w(lay.linear2.bias), lambda t: m(2, t))
        return F.layer_norm(x + m(3, y), d, w(lay.norm2.weight), w(lay.norm2.bias), lay.norm2.eps)
    h = m(2, torch.relu(x @ w(lay.linear1.weight).T + w(lay.linear1.bias)))
    return F.layer_norm(x + m(3, h @ w(lay.linear2.weight).T + w(lay.linear2.bias)), d, w(lay.norm2.weight), w(lay.norm2.bias), lay.norm2.eps)


class OutputCache:
    """The output buffers a device network owns: one set per (factory, N, stream), overwritten by the next call with the same N
    on the same stream, so that after the first call per (N, stream) a call neither allocates nor synchronises."""

    def __init__(self, name, device):
        self.name, self.device, self._bufs = name, device, {}

    def rows(self, boards):
        """N of uint8 (N,16) boards on the network's device."""
        L.require_device_tensor(boards, torch.uint8, (16,), "boards")
        if boards.device != self.device:
            raise ValueError("%s: boards on %s, weights on %s" % (self.name, boards.device, self.device))
        return boards.shape[0]

    def get(self, n, make):
        """make(n, device)'s buffers for n rows on the current stream."""
        key = (make, n, torch.cuda.current_stream(self.device).cuda_stream)
        bufs = self._bufs.get(key)
        if bufs is None:
            bufs = self._bufs[key] = make(n, self.device)
        return bufs


class PackedNet:
    """Base of DeviceTransformerPolicy and DeviceQNetwork: the module parsed, its parameters flattened into `plain` and packed
    into `packed` on its device, refresh() to redo both IN PLACE on the current stream, the output buffers, and the learner's side
    of both networks: `grad` (a buffer laid out like `plain`, filled by the subclass's loss_and_grad), attach_grads() and
    attach_params() (the module's gradients and parameters as views of the two buffers), and the optimiser's moments `exp_avg` and
    `exp_avg_sq` with _plain_changed() for the subclass's device step. A subclass gives name and, as
    staticmethods, parse and ops' plain_floats, packed_bytes and pack of its network."""

    name = parse = plain_floats = packed_bytes = pack = None

    def __init__(self, model, precision="f32"):
        if precision not in ops.POLICY_PRECISIONS:
            raise ValueError("%s: precision must be 'f32' or 'bf16'" % self.name)
        self.model, self.precision = model, precision
        self.parsed = self.parse(model)
        self.dim_ff, self.n_layers = self.parsed.dim_ff, len(self.parsed.layers)
        self.device = self.parsed.embedding.weight.device
        if self.device.type != "cuda":
            raise RuntimeError("g2048: %s needs the module on a ROCm device (got %s); there is no CPU path" % (self.name, self.device))
        self.plain = torch.empty(self.plain_floats(self.dim_ff, self.n_layers), dtype=torch.float32, device=self.device)
        self.packed = torch.empty(self.packed_bytes(precision, self.dim_ff, self.n_layers), dtype=torch.uint8, device=self.device)
        self._out = OutputCache(self.name, self.device)
        self.refresh()

    def refresh(self):
        if any(m.training for m in self.model.modules()):
            raise ValueError("%s.refresh: %s is in training mode; call .eval() first" % (self.name, type(self.model).__name__))
        if not self.params_attached:
            flatten(self.parsed, self.plain)
        self.pack(self.plain, self.dim_ff, self.n_layers, self.precision, out=self.packed)

    # ---- the learner's side: a gradient buffer in plain's layout, and the module's parameters and gradients as views
    @property
    def grad(self):
        """The gradient buffer loss_and_grad fills: float32 of plain.numel(), laid out like `plain` (allocated on first use)."""
        g = self.__dict__.get("_grad")
        if g is None:
            g = self.__dict__["_grad"] = torch.zeros_like(self.plain)
        return g

    def _moment(self, key):
        t = self.__dict__.get(key)
        if t is None:
            t = self.__dict__[key] = torch.zeros_like(self.plain)
        return t

    @property
    def exp_avg(self):
        """The optimiser's first moment of the subclass's device step: float32 of plain.numel(), laid out like `plain` (zeros,
        allocated on first use)."""
        return self._moment("_exp_avg")

    @property
    def exp_avg_sq(self):
        """The optimiser's second moment, like exp_avg."""
        return self._moment("_exp_avg_sq")

    def _plain_changed(self):
        """After net.plain was written on the device: the packed blob, and the module unless it is the plain buffer."""
        self.pack(self.plain, self.dim_ff, self.n_layers, self.precision, out=self.packed)
        if not self.params_attached:
            unflatten(self.parsed, self.plain)

    def attach_grads(self):
        """Sets every parameter's .grad of the module to a view into net.grad, at the offsets of flatten: from then on
        loss_and_grad, clip_grad_norm_(model.parameters(), ..), optimizer.step() and net.refresh() form a whole update with no
        gradient copy. Keep the optimizer's zero_grad(set_to_none=False), or call attach_grads() again after it."""
        o = 0
        for t in self.parsed.plain_tensors():
            if isinstance(t, torch.Tensor):
                t.grad = self.grad[o:o + t.numel()].view(t.shape)
                o += t.numel()
            else:
                o += 1
        return self.grad

    _attached = None        # attach_params(): (parameter, offset in floats) of the first and the last parameter

    @property
    def params_attached(self):
        """True while the module's parameters are the views attach_params() made (the first and the last are looked at)."""
        if self._attached is None:
            return False
        base = self.plain.data_ptr()
        return all(t.data_ptr() == base + 4 * o for t, o in self._attached)

    @torch.no_grad()
    def attach_params(self):
        """Rebinds the storage of every parameter of net.model to a view into net.plain, at the offsets of flatten (the
        counterpart of attach_grads): from then on the module IS the plain buffer. load_state_dict and an optimizer write
        through, a device-side update of net.plain needs no copy back into the module, and refresh() skips the re-flatten and only
        packs. The parameters' current values are kept. model.to(...), .float() or anything else that gives the parameters
        new storage undoes the attachment (refresh() then re-flattens again, as before); call attach_params() again after
        it. Returns net.plain."""
        flatten(self.parsed, self.plain)
        pairs, o = [], 0
        for t in self.parsed.plain_tensors():
            if isinstance(t, torch.Tensor):
                t.data = self.plain[o:o + t.numel()].view(t.shape)
                pairs.append((t, o))
                o += t.numel()
            else:
                o += 1
        self._attached = (pairs[0], pairs[-1])
        return self.plain
