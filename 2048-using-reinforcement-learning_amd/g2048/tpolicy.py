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
    must be back in eval mode): graphs captured earlier replay with the new weights.

    takes_boards = True: RolloutCollector hands it the packed boards instead of the float observations."""

    takes_boards = True
    name, parse = NAME, staticmethod(parse)
    plain_floats, packed_bytes, pack = map(staticmethod, (ops.tpolicy_plain_floats, ops.tpolicy_packed_bytes, ops.tpolicy_pack))

    def __call__(self, boards):
        probs, value = self._out.get(self._out.rows(boards), _outputs)
        return ops.tpolicy_forward(boards, self.packed, self.dim_ff, self.n_layers, self.precision, probs=probs, value=value)
