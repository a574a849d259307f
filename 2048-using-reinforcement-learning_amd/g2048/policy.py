"""The reference's PPO actor / critic (agents/ppo_agent.py:61-136, eval mode) as one HIP launch on the packed boards.

`DevicePolicy(actor, critic=None, precision="f32", batchnorm="auto")` takes the torch modules, folds every eval-mode
BatchNorm1d into a Linear (in f64, with torch ops on the modules' device, then cast to f32), packs the result with
`g2048_policy_pack` and runs `g2048_policy_forward` on uint8 (N,16) boards. Accepted layouts:

* the reference's: attributes fc1..fc4 (Linear) and bn1, bn2 (BatchNorm1d) with h1 = bn1(relu(fc1 x)), h2 = bn2(relu(fc2 h1)),
  h3 = relu(fc3 h2), out = fc4 h3 -- both BatchNorms skipped for a batch of one row, as the reference's forward does;
* an nn.Sequential (nested ones are flattened) of Linear / ReLU / BatchNorm1d / Dropout / Softmax with widths
  16-256-128-64-{4|1}: a BatchNorm right after a Linear folds into that Linear, one after a ReLU into the next Linear.

The actor's four outputs always go through the softmax. Anything else raises ValueError; a module in training mode is refused
(Dropout and batch-statistics BatchNorm have no device counterpart).
"""
import torch
import torch.nn as nn

from . import ops
from ._encoder_net import OutputCache

WIDTHS = (16, 256, 128, 64)
BATCHNORM_MODES = ("auto", "always", "never")


class _Layer:
    __slots__ = ("linear", "bn_in", "bn_out")

    def __init__(self, linear):
        self.linear, self.bn_in, self.bn_out = linear, None, None


def _check_bn(bn, width, where):
    if not isinstance(bn, nn.BatchNorm1d):
        raise ValueError("DevicePolicy: %s must be a BatchNorm1d" % where)
    if bn.num_features != width:
        raise ValueError("DevicePolicy: %s has %d features, the layer has %d" % (where, bn.num_features, width))
    if not bn.track_running_stats or bn.running_mean is None:
        raise ValueError("DevicePolicy: %s keeps no running statistics (batch statistics have no device counterpart)" % where)


def _check_widths(layers, n_out):
    if len(layers) != 4:
        raise ValueError("DevicePolicy: expected 4 Linear layers (16-256-128-64-%d), got %d" % (n_out, len(layers)))
    for i, lay in enumerate(layers):
        want = (WIDTHS[i], WIDTHS[i + 1] if i < 3 else n_out)
        got = (lay.linear.in_features, lay.linear.out_features)
        if got != want:
            raise ValueError("DevicePolicy: Linear %d is %d->%d, expected %d->%d" % (i + 1, got[0], got[1], want[0], want[1]))
        if lay.linear.bias is None:
            raise ValueError("DevicePolicy: Linear %d has no bias" % (i + 1))
    for i, lay in enumerate(layers):
        for bn, width, where in ((lay.bn_in, lay.linear.in_features, "the BatchNorm before Linear %d" % (i + 1)),
                                 (lay.bn_out, lay.linear.out_features, "the BatchNorm after Linear %d" % (i + 1))):
            if bn is not None:
                _check_bn(bn, width, where)


def _flatten(seq):
    for m in seq:
        if isinstance(m, nn.Sequential):
            yield from _flatten(m)
        else:
            yield m


def parse(module, n_out):
    """The network as four _Layer records plus whether it follows the reference's batch-of-one rule. Raises ValueError."""
    if not isinstance(module, nn.Module):
        raise ValueError("DevicePolicy: expected a torch.nn.Module, got %s" % type(module).__name__)
    if any(m.training for m in module.modules()):
        raise ValueError("DevicePolicy: %s is in training mode; call .eval() first (inference only)" % type(module).__name__)
    names = dict(module.named_children())
    if all(k in names for k in ("fc1", "fc2", "fc3", "fc4", "bn1", "bn2")) and not isinstance(module, nn.Sequential):
        if not all(isinstance(names["fc%d" % i], nn.Linear) for i in range(1, 5)):
            raise ValueError("DevicePolicy: fc1..fc4 must be Linear layers")
        layers = [_Layer(names["fc%d" % i]) for i in range(1, 5)]
        layers[1].bn_in, layers[2].bn_in = names["bn1"], names["bn2"]       # relu -> bn -> (dropout) -> next fc
        _check_widths(layers, n_out)
        return layers, True
    if not isinstance(module, nn.Sequential):
        raise ValueError("DevicePolicy: %s is neither the reference's fc1..fc4 / bn1, bn2 layout nor an nn.Sequential"
                         % type(module).__name__)
    layers, prev, pending_bn, relus, softmax = [], None, None, 0, False
    for m in _flatten(module):
        if softmax:
            raise ValueError("DevicePolicy: Softmax must be the last layer")
        if isinstance(m, nn.Dropout):
            continue
        if isinstance(m, nn.Linear):
            if layers and relus != len(layers):
                raise ValueError("DevicePolicy: Linear %d is not preceded by a ReLU" % (len(layers) + 1))
            layers.append(_Layer(m))
            layers[-1].bn_in, pending_bn = pending_bn, None
            prev = "linear"
        elif isinstance(m, nn.BatchNorm1d):
            if prev == "linear" and layers[-1].bn_out is None:
                layers[-1].bn_out = m
            elif prev == "relu" and pending_bn is None:
                pending_bn = m
            else:
                raise ValueError("DevicePolicy: a BatchNorm1d must follow a Linear or a ReLU (one each)")
            prev = "bn"
        elif isinstance(m, nn.ReLU):
            if not layers or relus == len(layers) or len(layers) == 4:
                raise ValueError("DevicePolicy: ReLU in an unexpected place (one after each of the first three Linears)")
            relus += 1
            prev = "relu"
        elif isinstance(m, nn.Softmax):
            if len(layers) != 4 or prev != "linear" or m.dim not in (-1, 1):
                raise ValueError("DevicePolicy: Softmax must follow the last Linear, over dim -1")
            softmax = True
        else:
            raise ValueError("DevicePolicy: unsupported layer %s" % type(m).__name__)
    if pending_bn is not None:
        raise ValueError("DevicePolicy: a trailing BatchNorm1d has no Linear to fold into")
    if relus != 3:
        raise ValueError("DevicePolicy: expected a ReLU after each of the first three Linears")
    if softmax and n_out != 4:
        raise ValueError("DevicePolicy: the critic must not end in Softmax")
    _check_widths(layers, n_out)
    return layers, False


def _bn_affine(bn):
    s = torch.rsqrt(bn.running_var.double() + bn.eps)
    if bn.weight is not None:
        s = s * bn.weight.double()
    t = -bn.running_mean.double() * s
    if bn.bias is not None:
        t = t + bn.bias.double()
    return s, t


@torch.no_grad()
def fold(layers, apply_bn=True):
    """[(W f64 [out][in], b f64 [out])] * 4 of the network with every BatchNorm folded in (apply_bn) or dropped."""
    out = []
    for lay in layers:
        W, b = lay.linear.weight.double(), lay.linear.bias.double()
        if apply_bn and lay.bn_in is not None:          # Linear(s * x + t) = (W diag s) x + (b + W t)
            s, t = _bn_affine(lay.bn_in)
            b = b + W @ t
            W = W * s[None, :]
        if apply_bn and lay.bn_out is not None:         # s * (W x + b) + t
            s, t = _bn_affine(lay.bn_out)
            W = W * s[:, None]
            b = b * s + t
        out.append((W, b))
    return out


def forward_reference(folded, x, softmax):
    """The folded network on float observations in f64 with torch ops (any device): the CPU yardstick of the kernel."""
    h = x.double()
    for i, (W, b) in enumerate(folded):
        h = h @ W.T + b
        if i < 3:
            h = torch.relu(h)
    return torch.softmax(h, -1) if softmax else h


class _Net:
    """One network on the device: the plain f32 parameter buffer(s) and the packed blob(s), with and without BatchNorm."""

    def __init__(self, module, n_out, precision, batchnorm):
        self.module, self.n_out, self.precision = module, n_out, precision
        self.layers, self.reference_rule = parse(module, n_out)
        self.device = self.layers[0].linear.weight.device
        if self.device.type != "cuda":
            raise RuntimeError("g2048: DevicePolicy needs the modules on a ROCm device (got %s); there is no CPU path" % self.device)
        has_bn = any(l.bn_in is not None or l.bn_out is not None for l in self.layers)
        if batchnorm == "never" or not has_bn:
            sets = {"off": False}
        elif batchnorm == "always" or not self.reference_rule:
            sets = {"on": True}          # torch's eval forward of a Sequential applies BatchNorm at every batch size
        else:
            sets = {"on": True, "off": False}
        self.sets = sets
        nplain = 45504 + 65 * n_out
        self.plain = {k: torch.empty(nplain, dtype=torch.float32, device=self.device) for k in sets}
        self.packed = {k: torch.empty(ops.policy_packed_bytes(precision, n_out), dtype=torch.uint8, device=self.device) for k in sets}
        self.refresh()

    @torch.no_grad()
    def refresh(self):
        if any(m.training for m in self.module.modules()):
            raise ValueError("DevicePolicy.refresh: %s is in training mode; call .eval() first" % type(self.module).__name__)
        for key, apply_bn in self.sets.items():
            plain, o = self.plain[key], 0
            for W, b in fold(self.layers, apply_bn):
                for p in (W, b):
                    plain[o:o + p.numel()].copy_(p.reshape(-1))       # f64 -> f32 (round to nearest) in the copy
                    o += p.numel()
            ops.policy_pack(plain, self.n_out, self.precision, out=self.packed[key])

    def blob(self, n):
        if len(self.sets) == 1:
            return next(iter(self.packed.values()))
        return self.packed["on" if n > 1 else "off"]


class DevicePolicy:
    """PPO policy network on the device: __call__(boards uint8 (N,16)) -> probs float32 (N,4), or (probs, value float32 (N,1))
    when a critic is given. One g2048_policy_forward launch per call; the outputs are buffers owned by the policy (one pair per
    (N, stream), overwritten by the next call with the same N on the same stream), so after the first call per (N, stream) a
    call neither allocates nor synchronises and can be captured in a graph (RolloutCollector does).

    precision: "f32" (exact f32 MFMA, the parity path) or "bf16" (bf16 weights and activations, f32 accumulation and softmax).
    batchnorm: "auto" follows each module's own eval forward (the reference's layout skips BatchNorm for a batch of one row, so
    both folded and unfolded weights are kept; a Sequential applies it always), "always" / "never" force it.
    refresh() re-folds and re-packs the weights IN PLACE on the current stream (call it after an optimizer step; the module
    must be back in eval mode): graphs captured earlier replay with the new weights.

    takes_boards = True: RolloutCollector hands it the packed boards instead of the float observations."""

    takes_boards = True

    def __init__(self, actor, critic=None, precision="f32", batchnorm="auto"):
        if precision not in ops.POLICY_PRECISIONS:
            raise ValueError("DevicePolicy: precision must be 'f32' or 'bf16'")
        if batchnorm not in BATCHNORM_MODES:
            raise ValueError("DevicePolicy: batchnorm must be one of %s" % (BATCHNORM_MODES,))
        self.precision, self.batchnorm = precision, batchnorm
        self.actor = _Net(actor, 4, precision, batchnorm)
        self.critic = _Net(critic, 1, precision, batchnorm) if critic is not None else None
        if self.critic is not None and self.critic.device != self.actor.device:
            raise ValueError("DevicePolicy: actor and critic live on different devices")
        self.device = self.actor.device
        self._out = OutputCache("DevicePolicy", self.device)

    def refresh(self):
        self.actor.refresh()
        if self.critic is not None:
            self.critic.refresh()

    def _outputs(self, n, device):
        return (torch.empty((n, 4), dtype=torch.float32, device=device),
                torch.empty((n, 1), dtype=torch.float32, device=device) if self.critic is not None else None)

    def __call__(self, boards):
        n = self._out.rows(boards)
        probs, value = self._out.get(n, self._outputs)
        return ops.policy_forward(boards, self.actor.blob(n), self.critic.blob(n) if self.critic is not None else None,
                                  self.precision, probs=probs, value=value)
