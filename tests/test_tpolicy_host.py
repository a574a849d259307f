"""CPU-side checks of g2048.DeviceTransformerPolicy: the hash-derived weights against the checksums recorded in
tests/golden/tpolicy.npz, a stock-torch module of the reference's structure on them against the reference class's recorded
f64 outputs, the conditions that make the fixture pin something, the structural parse (three spellings accepted, every
unsupported variant refused with its reason), the plain-layout round trip and the C-ABI's argument validation. The kernel
itself is checked on the GPU (tests/test_gpu_tpolicy.py)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import tpolicy_weights as tw
from conftest import load_golden


class RefSpelling(nn.Module):
    """The structure and attribute names of the reference's TransformerModel (models/transformer.py:4-40), built from stock
    torch modules; dim_ff and the layer keyword arguments are open so that the refusals can be provoked."""

    def __init__(self, dim_ff=2048, num_layers=2, d_model=64, nhead=4, final_norm=False, **layer_kw):
        super().__init__()
        self.embedding = nn.Linear(1, d_model)
        layer = nn.TransformerEncoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=dim_ff, **{"batch_first": True, **layer_kw})
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=num_layers, enable_nested_tensor=False,
                                                         norm=nn.LayerNorm(d_model) if final_norm else None)
        self.fc1, self.fc2 = nn.Linear(d_model * 16, 128), nn.Linear(128, 64)
        self.actor, self.critic = nn.Linear(64, 4), nn.Linear(64, 1)

    def forward(self, x):
        n = x.size(0)
        x = self.transformer_encoder(self.embedding(x.view(n, 16, 1))).reshape(n, -1)
        x = torch.relu(self.fc2(torch.relu(self.fc1(x))))
        return torch.softmax(self.actor(x), dim=-1), self.critic(x)


class BenchSpelling(nn.Module):
    """bench.py's config-4 policy: emb / enc / fc (Sequential)."""

    def __init__(self, dim_ff=128, num_layers=2):
        super().__init__()
        self.emb = nn.Linear(1, 64)
        self.enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(64, 4, dim_ff, batch_first=True), num_layers)
        self.fc = nn.Sequential(nn.Linear(1024, 128), nn.ReLU(), nn.Linear(128, 64), nn.ReLU())
        self.actor, self.critic = nn.Linear(64, 4), nn.Linear(64, 1)

    def forward(self, x):
        h = self.fc(self.enc(self.emb(x.view(x.shape[0], 16, 1))).reshape(x.shape[0], -1))
        return torch.softmax(self.actor(h), -1), self.critic(h)


class RolloutSpelling(nn.Module):
    """tests/test_gpu_rollout.py's TinyTransformerPolicy: embedding / encoder / fc."""

    def __init__(self, dim_ff=128, num_layers=2):
        super().__init__()
        self.embedding = nn.Linear(1, 64)
        layer = nn.TransformerEncoderLayer(d_model=64, nhead=4, dim_feedforward=dim_ff, batch_first=True)
        self.encoder = nn.TransformerEncoder(layer, num_layers=num_layers)
        self.fc = nn.Sequential(nn.Linear(1024, 128), nn.ReLU(), nn.Linear(128, 64), nn.ReLU())
        self.actor, self.critic = nn.Linear(64, 4), nn.Linear(64, 1)

    def forward(self, x):
        h = self.encoder(self.embedding(x.view(x.shape[0], 16, 1)))
        h = self.fc(h.reshape(x.shape[0], -1))
        return torch.softmax(self.actor(h), dim=-1), self.critic(h)


def golden_model():
    """(fixture, RefSpelling in float64 eval mode carrying the fixture's hash-derived weights)."""
    g = load_golden("tpolicy.npz")
    dim_ff, n_layers = int(g["dim_ff"]), int(g["n_layers"])
    model = RefSpelling(dim_ff, n_layers).double()
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert shapes == tw.reference_shapes(dim_ff, n_layers)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in tw.state_dict(shapes).items()})
    return g, model.eval()


def scale_heads(model, gain=8.0):
    """torch's default init gives near-uniform probabilities for every board; larger heads make the outputs depend on it."""
    with torch.no_grad():
        model.actor.weight.mul_(gain)
        model.critic.weight.mul_(gain)
    return model


def bf16_round(t):
    return t.float().bfloat16().to(t.dtype)


def test_hash_weights_reproduce_the_recorded_checksums():
    g = load_golden("tpolicy.npz")
    assert dict(zip(g["recipe_names"].tolist(), g["recipe_values"].tolist())) == tw.RECIPE
    shapes = tw.reference_shapes(int(g["dim_ff"]), int(g["n_layers"]))
    assert [k for k, _ in shapes] == g["tensor_names"].tolist()
    sd = tw.state_dict(shapes)
    assert sum(v.size for v in sd.values()) == 702213
    assert [tw.checksum(sd[k]) for k, _ in shapes] == g["tensor_crc32"].tolist()
    for v in sd.values():
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), "a weight is not exact in float32"


def test_stock_torch_module_on_the_hash_weights_equals_the_reference_class():
    from g2048 import tpolicy
    g, model = golden_model()
    x = torch.from_numpy(g["boards"]).double() / 15
    with torch.no_grad():
        p, v = model(x)
    ep, ev = np.abs(p.numpy() - g["probs_f64"]).max(), np.abs(v.numpy() - g["value_f64"]).max()
    print("module vs recorded f64: probs %.3g values %.3g" % (ep, ev))
    assert ep <= 1e-12 and ev <= 1e-12
    # the converter's own f64 forward (what the GPU tests compare the kernel with at other shapes) is the same function
    p2, v2 = tpolicy.forward_reference(tpolicy.parse(model), torch.from_numpy(g["boards"]))
    assert np.abs(p2.numpy() - g["probs_f64"]).max() <= 1e-12 and np.abs(v2.numpy() - g["value_f64"]).max() <= 1e-12
    p3, v3 = tpolicy.forward_reference(tpolicy.parse(model), torch.from_numpy(g["boards"]), round_weights=bf16_round)
    assert np.abs(p3.numpy() - g["probs_bf16w"]).max() <= 1e-12 and np.abs(v3.numpy() - g["value_bf16w"]).max() <= 1e-12


def test_fixture_outputs_depend_on_the_board():
    g = load_golden("tpolicy.npz")
    assert g["boards"].shape == (2048, 16) and np.array_equal(g["boards"], load_golden("policy.npz")["boards"])
    p = g["probs_f64"]
    top, counts = p.max(1), np.bincount(p.argmax(1), minlength=4)
    assert top.min() < 0.5 and top.max() > 0.9
    assert (counts >= 0.1 * len(p)).sum() >= 2
    assert np.abs(g["probs_f32"] - p).max() < 2e-5 and np.abs(g["probs_bf16w"] - p).max() > 1e-4


@pytest.mark.parametrize("spelling", [RefSpelling, BenchSpelling, RolloutSpelling])
def test_parse_accepts_the_three_spellings(spelling):
    from g2048 import tpolicy
    torch.manual_seed(3)
    model = scale_heads(spelling(dim_ff=96, num_layers=3).eval())
    p = tpolicy.parse(model)
    assert p.dim_ff == 96 and len(p.layers) == 3
    assert (p.embedding.in_features, p.fc1.in_features, p.fc2.in_features, p.actor.out_features, p.critic.out_features) == (1, 1024, 128, 4, 1)
    b = torch.randint(0, 16, (64, 16), dtype=torch.uint8)
    with torch.no_grad():
        want_p, want_v = model.double()(b.double() / 15)
    got_p, got_v = tpolicy.forward_reference(p, b)
    assert (got_p - want_p).abs().max() <= 1e-12 and (got_v - want_v).abs().max() <= 1e-12


def test_parse_refuses_what_the_kernel_cannot_run():
    from g2048 import DeviceTransformerPolicy, tpolicy
    torch.manual_seed(4)
    with pytest.raises(ValueError, match="training mode"):
        tpolicy.parse(RefSpelling(128))                         # a fresh module is in training mode
    with pytest.raises(ValueError, match="norm_first"):
        tpolicy.parse(RefSpelling(128, norm_first=True).eval())
    with pytest.raises(ValueError, match="activation other than ReLU"):
        tpolicy.parse(RefSpelling(128, activation="gelu").eval())
    with pytest.raises(ValueError, match="batch_first=False"):
        tpolicy.parse(RefSpelling(128, batch_first=False).eval())
    with pytest.raises(ValueError, match="d_model 32"):
        m = RefSpelling(128, d_model=32).eval()
        m.embedding, m.fc1 = nn.Linear(1, 64), nn.Linear(1024, 128)     # the Linears outside are as expected: the encoder is not
        tpolicy.parse(m.eval())
    with pytest.raises(ValueError, match="nhead 8"):
        tpolicy.parse(RefSpelling(128, nhead=8).eval())
    with pytest.raises(ValueError, match="dim_ff 48, not a multiple of 32"):
        tpolicy.parse(RefSpelling(48).eval())
    with pytest.raises(ValueError, match="final norm"):
        tpolicy.parse(RefSpelling(128, final_norm=True).eval())
    with pytest.raises(ValueError, match="missing bias"):
        tpolicy.parse(RefSpelling(128, bias=False).eval())
    m = RefSpelling(128).eval()
    m.fc2 = nn.Linear(128, 64, bias=False)
    with pytest.raises(ValueError, match="fc2 Linear 128->64 has a missing bias"):
        tpolicy.parse(m.eval())
    m = RefSpelling(128).eval()
    del m.critic
    with pytest.raises(ValueError, match=r"missing Linear 64->1 \(critic\)"):
        tpolicy.parse(m.eval())
    m = RefSpelling(128).eval()
    m.actor2 = nn.Linear(64, 4)
    with pytest.raises(ValueError, match="duplicate Linear 64->4"):
        tpolicy.parse(m.eval())
    m = RefSpelling(128).eval()
    m.extra = nn.Linear(64, 7)
    with pytest.raises(ValueError, match="unexpected Linear 64->7"):
        tpolicy.parse(m.eval())
    with pytest.raises(ValueError, match="exactly one nn.TransformerEncoder, found 0"):
        tpolicy.parse(nn.Sequential(nn.Linear(1, 64)).eval())
    m = RefSpelling(128).eval()
    m.second = nn.TransformerEncoder(nn.TransformerEncoderLayer(64, 4, 128, batch_first=True), 1).eval()
    with pytest.raises(ValueError, match="found 2"):
        tpolicy.parse(m.eval())
    with pytest.raises(ValueError, match="torch.nn.Module"):
        tpolicy.parse("model")
    ok = RefSpelling(128).eval()
    with pytest.raises(ValueError, match="precision"):
        DeviceTransformerPolicy(ok, precision="f16")
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeviceTransformerPolicy(ok)                             # the module lives on the CPU


def test_plain_layout_round_trips():
    from g2048 import ops, tpolicy
    torch.manual_seed(5)
    a, b = BenchSpelling(64, 3).eval(), BenchSpelling(64, 3).eval()
    pa, pb = tpolicy.parse(a), tpolicy.parse(b)
    pa.layers[1].norm2.eps = 3e-4
    plain = tpolicy.flatten(pa)
    assert plain.dtype == torch.float32 and plain.numel() == ops.tpolicy_plain_floats(64, 3) == 128 + 3 * (16962 + 129 * 64) + 139781
    # the documented offsets: embedding first, eps after each layer's four norm vectors, the critic's bias last
    layer = 16962 + 129 * 64
    assert torch.equal(plain[:64], a.emb.weight.detach().reshape(-1)) and plain[-1] == a.critic.bias.detach()[0]
    assert plain[128 + layer - 2] == np.float32(1e-5) and plain[128 + 2 * layer - 1] == np.float32(3e-4)
    assert torch.equal(plain[128 + 2 * layer:128 + 2 * layer + 192 * 64], a.enc.layers[2].self_attn.in_proj_weight.detach().reshape(-1))
    tpolicy.unflatten(pb, plain)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    assert torch.equal(tpolicy.flatten(pb)[:128 + layer - 2], plain[:128 + layer - 2])
    assert ops.tpolicy_plain_floats(2048, 2) == 702213 + 4


def test_tpolicy_entry_points_validate_without_device():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    L = _lib.lib()
    f32, bf16 = L.g2048_tpolicy_packed_bytes(0, 2048, 2), L.g2048_tpolicy_packed_bytes(1, 2048, 2)
    assert 2.8e6 < f32 < 3.0e6 and 1.4e6 < bf16 < 1.5e6 and f32 % 16 == 0 and bf16 % 16 == 0
    assert 0.8e6 < L.g2048_tpolicy_packed_bytes(0, 128, 2) < 0.85e6
    assert L.g2048_tpolicy_packed_bytes(0, 128, 3) - L.g2048_tpolicy_packed_bytes(0, 128, 2) == 128 * 1024 + (128 + 580) * 4
    for bad in ((2, 128, 2), (0, 48, 2), (0, 0, 2), (0, 128, 0), (0, -32, 1)):
        assert L.g2048_tpolicy_packed_bytes(*bad) == 0, bad
    buf = (C.c_uint8 * 256)()
    a = (C.addressof(buf) + 15) & ~15
    assert L.g2048_tpolicy_forward(None, None, None, None, 0, 128, 2, 0, None) == 0          # n == 0: nothing to do
    assert L.g2048_tpolicy_forward(None, a, a, None, 8, 128, 2, 0, None) == -1 and b"null pointer" in L.g2048_last_error()
    assert L.g2048_tpolicy_forward(a + 4, a, a, None, 8, 128, 2, 0, None) == -1 and b"misaligned" in L.g2048_last_error()
    assert L.g2048_tpolicy_forward(a, a, a, a + 2, 8, 128, 2, 0, None) == -1 and b"misaligned" in L.g2048_last_error()
    assert L.g2048_tpolicy_forward(a, a, a, None, 8, 128, 2, 2, None) == -1 and b"opts" in L.g2048_last_error()
    assert L.g2048_tpolicy_forward(a, a, a, None, 8, 48, 2, 0, None) == -1 and b"dim_ff" in L.g2048_last_error()
    assert L.g2048_tpolicy_forward(a, a, a, None, 8, 128, 0, 0, None) == -1 and b"n_layers" in L.g2048_last_error()
    assert L.g2048_tpolicy_pack(None, 128, 2, 0, a, None) == -1 and b"null pointer" in L.g2048_last_error()
    assert L.g2048_tpolicy_pack(a, 128, 2, 7, a, None) == -1 and b"precision" in L.g2048_last_error()
    assert L.g2048_tpolicy_pack(a, 48, 2, 0, a, None) == -1 and b"dim_ff" in L.g2048_last_error()
    assert L.g2048_tpolicy_pack(a, 128, 2, 0, a + 8, None) == -1 and b"misaligned" in L.g2048_last_error()
