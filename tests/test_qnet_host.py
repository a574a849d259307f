"""CPU-side checks of g2048.DeviceQNetwork: the hash-derived weights against the checksums recorded in tests/golden/qnet.npz, a
stock-torch module of the reference's structure on them against the reference class's recorded per-board f64 outputs, the
sequence quirk (a batch call of the module is NOT the per-board function), the conditions that make the fixture pin something,
the structural parse (every unsupported variant refused with its reason), the plain layout against the state dict and the
C-ABI's size arithmetic and argument validation. The kernel itself is checked on the GPU (tests/test_gpu_qnet.py)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import qnet_weights as qw
from conftest import load_golden


class RefSpelling(nn.Module):
    """The structure and attribute names of the reference's HybridDQN (agents/hybrid.py:700-727), built from stock torch
    modules; dim_ff, the layer keyword arguments and the convolutions' arguments are open so that the refusals can be provoked.
    forward() is the reference's: the encoder sees x.unsqueeze(1), one sequence of B tokens unless batch_first is set."""

    def __init__(self, dim_ff=2048, num_layers=2, d_model=128, nhead=8, final_norm=False, conv1_kw=None, conv2_kw=None, **layer_kw):
        super().__init__()
        self.cnn = nn.Sequential(nn.Conv2d(1, 32, **{"kernel_size": 2, "stride": 1, "padding": 1, **(conv1_kw or {})}), nn.ReLU(),
                                 nn.Conv2d(32, 64, **{"kernel_size": 2, "stride": 1, "padding": 0, **(conv2_kw or {})}), nn.ReLU())
        self.embedding = nn.Linear(64 * 4 * 4, 128)
        layer = nn.TransformerEncoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=dim_ff, **layer_kw)
        self.transformer = nn.TransformerEncoder(layer, num_layers=num_layers, enable_nested_tensor=False,
                                                 norm=nn.LayerNorm(d_model) if final_norm else None)
        self.fc = nn.Linear(128, 4)

    def forward(self, x):
        n = x.shape[0]
        x = self.embedding(self.cnn(x.view(-1, 1, 4, 4)).view(n, -1))
        return self.fc(self.transformer(x.unsqueeze(1)).squeeze(1))


class OtherSpelling(nn.Module):
    """Other names, a batch_first encoder with 4 heads, the convolutions as attributes: the same per-board function."""

    def __init__(self, dim_ff=64, num_layers=2):
        super().__init__()
        self.c1, self.c2 = nn.Conv2d(1, 32, 2, padding=1), nn.Conv2d(32, 64, 2)
        self.emb = nn.Linear(1024, 128)
        self.enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(128, 4, dim_ff, batch_first=True), num_layers, enable_nested_tensor=False)
        self.head = nn.Sequential(nn.Linear(128, 4))

    def forward(self, x):
        n = x.shape[0]
        h = torch.relu(self.c2(torch.relu(self.c1(x.view(-1, 1, 4, 4))))).reshape(n, -1)
        return self.head(self.enc(self.emb(h).unsqueeze(1)).squeeze(1))


def tiles(boards, dtype=torch.float64):
    """uint8 codes as the env's get_state(): 2 ** code, 0 for empty."""
    b = np.asarray(boards)
    return torch.from_numpy(np.where(b > 0, 2.0 ** b.astype(np.float64), 0.0)).to(dtype)


def per_board(model, x):
    """The module one board per call, the only way the reference calls it."""
    with torch.no_grad():
        return torch.cat([model(x[i:i + 1]) for i in range(len(x))])


def golden_model():
    """(fixture, boards, RefSpelling in float64 eval mode carrying the fixture's hash-derived weights)."""
    g = load_golden("qnet.npz")
    dim_ff, n_layers = int(g["dim_ff"]), int(g["n_layers"])
    model = RefSpelling(dim_ff, n_layers).double()
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert shapes == qw.reference_shapes(dim_ff, n_layers)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in qw.state_dict(shapes).items()})
    return g, load_golden("policy.npz")["boards"], model.eval()


def bf16_round(t):
    return t.float().bfloat16().to(t.dtype)


def random_model(seed, dim_ff=64, num_layers=2, spelling=RefSpelling):
    """torch's default init, eval mode, on the CPU."""
    torch.manual_seed(seed)
    return spelling(dim_ff, num_layers).eval()


def test_hash_weights_reproduce_the_recorded_checksums():
    g = load_golden("qnet.npz")
    assert dict(zip(g["recipe_names"].tolist(), g["recipe_values"].tolist())) == qw.RECIPE
    shapes = qw.reference_shapes(int(g["dim_ff"]), int(g["n_layers"]))
    assert [k for k, _ in shapes] == g["tensor_names"].tolist()
    sd = qw.state_dict(shapes)
    assert sum(v.size for v in sd.values()) == qw.N_PARAMETERS == 1326180
    assert [qw.checksum(sd[k]) for k, _ in shapes] == g["tensor_crc32"].tolist()
    for v in sd.values():
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), "a weight is not exact in float32"


def test_forward_reference_is_the_modules_per_board_function_and_not_its_batch_call():
    from g2048 import qnet
    g, boards, model = golden_model()
    parsed = qnet.parse(model)
    q = qnet.forward_reference(parsed, torch.from_numpy(boards)).numpy()
    e = np.abs(q - g["q_f64"]).max()
    print("forward_reference vs the reference class's recorded per-board f64: %.3g" % e)
    assert e <= 1e-12
    qb = qnet.forward_reference(parsed, torch.from_numpy(boards), round_weights=bf16_round).numpy()
    assert np.abs(qb - g["q_bf16w"]).max() <= 1e-12
    x = tiles(boards[:512])
    one = per_board(model, x[:64]).numpy()                  # the stock module one board per call
    assert np.abs(one - g["q_f64"][:64]).max() <= 1e-12
    with torch.no_grad():                                   # the (1, B, 128) form is the same function ...
        h = model.embedding(model.cnn(x.view(-1, 1, 4, 4)).view(len(x), -1))
        alt = model.fc(model.transformer(h.unsqueeze(0)).squeeze(0)).numpy()
        batch = model(x).numpy()                            # ... and the module's own batch call is not: its boards attend to each other
    assert np.abs(alt - g["q_f64"][:512]).max() <= 1e-12
    quirk = np.abs(batch - g["q_f64"][:512]).max()
    print("model(x) on 512 boards vs the per-board function: %.3g (max|Q| %.3g)" % (quirk, np.abs(g["q_f64"]).max()))
    assert quirk > 1e-2


def test_fixture_pins_actions_and_stays_clear_of_ties(oracle):
    g, boards, _ = golden_model()
    assert boards.shape == (2048, 16) and boards.max() == 17
    q = g["q_f64"]
    valid = qw.mask_bits(oracle.valid_moves_batch(boards))
    assert np.array_equal(g["actions_f64"], qw.masked_argmax(q, valid))
    counts = np.bincount(g["actions_f64"], minlength=4)
    assert (counts >= 0.1 * len(q)).sum() >= 2, counts
    assert (~valid.any(1)).sum() > 0 and np.all(g["actions_f64"][~valid.any(1)] == 0)      # no valid move: action 0
    gap = qw.top_two_gap(q, valid)
    f32_bound, bf16_bound = 8 * np.abs(g["q_f32"] - q).max(), 4 * np.abs(g["q_bf16w"] - q).max()
    assert (gap <= 2 * f32_bound).mean() <= 0.01 and (gap <= 2 * bf16_bound).mean() <= 0.20
    qmax = np.abs(q).max()
    assert np.abs(g["q_f32"] - q).max() < 1e-5 * qmax and 1e-4 * qmax < np.abs(g["q_bf16w"] - q).max() < 2e-2 * qmax


def test_parse_accepts_other_spellings():
    from g2048 import qnet
    model = random_model(3, 96, 3, OtherSpelling)
    p = qnet.parse(model)
    assert p.dim_ff == 96 and len(p.layers) == 3
    assert (p.conv1.out_channels, p.conv2.out_channels, p.embedding.in_features, p.fc.out_features) == (32, 64, 1024, 4)
    b = torch.randint(0, 16, (48, 16), dtype=torch.uint8)
    want = per_board(model.double(), tiles(b.numpy()))
    assert (qnet.forward_reference(p, b) - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max()))
    p2 = qnet.parse(RefSpelling(64, 1, nhead=2).eval())      # nhead and batch_first are not constrained
    assert p2.dim_ff == 64 and len(p2.layers) == 1


def test_parse_refuses_what_the_kernel_cannot_run():
    from g2048 import DeviceQNetwork, qnet
    torch.manual_seed(4)
    with pytest.raises(ValueError, match="training mode"):
        qnet.parse(RefSpelling(64))                             # a fresh module is in training mode
    with pytest.raises(ValueError, match="norm_first"):
        qnet.parse(RefSpelling(64, norm_first=True).eval())
    with pytest.raises(ValueError, match="activation other than ReLU"):
        qnet.parse(RefSpelling(64, activation="gelu").eval())
    with pytest.raises(ValueError, match="d_model 64"):
        qnet.parse(RefSpelling(64, d_model=64).eval())
    with pytest.raises(ValueError, match="dim_ff 48, not a multiple of 32"):
        qnet.parse(RefSpelling(48).eval())
    with pytest.raises(ValueError, match="final norm"):
        qnet.parse(RefSpelling(64, final_norm=True).eval())
    with pytest.raises(ValueError, match="missing bias"):
        qnet.parse(RefSpelling(64, bias=False).eval())
    m = RefSpelling(64).eval()
    m.transformer.layers[1].linear1, m.transformer.layers[1].linear2 = nn.Linear(128, 32), nn.Linear(32, 128)
    with pytest.raises(ValueError, match="layer 1 has dim_ff 32, layer 0 has 64"):
        qnet.parse(m.eval())
    with pytest.raises(ValueError, match=r"Conv2d 1->32 needs zero padding 1"):
        qnet.parse(RefSpelling(64, conv1_kw={"padding": 0}).eval())
    with pytest.raises(ValueError, match=r"Conv2d 32->64 needs zero padding 0"):
        qnet.parse(RefSpelling(64, conv2_kw={"padding": 1}).eval())
    with pytest.raises(ValueError, match=r"Conv2d 1->32 needs kernel 2 and stride 1"):
        qnet.parse(RefSpelling(64, conv1_kw={"kernel_size": 3}).eval())
    with pytest.raises(ValueError, match=r"Conv2d 32->64 needs kernel 2 and stride 1"):
        qnet.parse(RefSpelling(64, conv2_kw={"stride": 2}).eval())
    with pytest.raises(ValueError, match=r"Conv2d 32->64 has a missing bias"):
        qnet.parse(RefSpelling(64, conv2_kw={"bias": False}).eval())
    m = RefSpelling(64).eval()
    m.cnn[2] = nn.Conv2d(32, 48, 2)
    with pytest.raises(ValueError, match="unexpected Conv2d 32->48"):
        qnet.parse(m.eval())
    m = RefSpelling(64).eval()
    m.cnn = nn.Sequential(m.cnn[0], nn.ReLU())
    with pytest.raises(ValueError, match=r"missing Conv2d 32->64 \(conv2\)"):
        qnet.parse(m.eval())
    m = RefSpelling(64).eval()
    m.again = nn.Conv2d(1, 32, 2, padding=1)
    with pytest.raises(ValueError, match="duplicate Conv2d 1->32"):
        qnet.parse(m.eval())
    m = RefSpelling(64).eval()
    m.fc = nn.Linear(128, 4, bias=False)
    with pytest.raises(ValueError, match="fc Linear 128->4 has a missing bias"):
        qnet.parse(m.eval())
    m = RefSpelling(64).eval()
    del m.fc
    with pytest.raises(ValueError, match=r"missing Linear 128->4 \(fc\)"):
        qnet.parse(m.eval())
    m = RefSpelling(64).eval()
    m.fc2 = nn.Linear(128, 4)
    with pytest.raises(ValueError, match="duplicate Linear 128->4"):
        qnet.parse(m.eval())
    m = RefSpelling(64).eval()
    m.extra = nn.Linear(128, 7)
    with pytest.raises(ValueError, match="unexpected Linear 128->7"):
        qnet.parse(m.eval())
    with pytest.raises(ValueError, match="exactly one nn.TransformerEncoder, found 0"):
        qnet.parse(nn.Sequential(nn.Linear(1024, 128)).eval())
    m = RefSpelling(64).eval()
    m.second = nn.TransformerEncoder(nn.TransformerEncoderLayer(128, 8, 64), 1, enable_nested_tensor=False).eval()
    with pytest.raises(ValueError, match="found 2"):
        qnet.parse(m.eval())
    with pytest.raises(ValueError, match="torch.nn.Module"):
        qnet.parse("model")
    ok = RefSpelling(64).eval()
    with pytest.raises(ValueError, match="precision"):
        DeviceQNetwork(ok, precision="f16")
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeviceQNetwork(ok)                                      # the module lives on the CPU


def test_flatten_follows_the_state_dict():
    from g2048 import ops, qnet
    model = random_model(5, 64, 3)
    p = qnet.parse(model)
    p.layers[1].norm2.eps = 3e-4
    plain = qnet.flatten(p)
    layer = 66690 + 257 * 64
    assert plain.dtype == torch.float32 and plain.numel() == ops.qnet_plain_floats(64, 3) == 140132 + 3 * layer
    # the state dict in its order, the two eps after each layer's four norm vectors
    o = 0
    for name, t in model.state_dict().items():
        assert torch.equal(plain[o:o + t.numel()], t.reshape(-1)), name
        o += t.numel()
        if name.endswith("norm2.bias"):
            l = int(name.split(".")[2])
            assert plain[o] == np.float32(1e-5) and plain[o + 1] == np.float32(3e-4 if l == 1 else 1e-5)
            o += 2
    assert o == plain.numel()
    assert ops.qnet_plain_floats(2048, 2) == 1326180 + 4
    # written in place when a buffer is given; a buffer of another size is refused
    buf = torch.zeros_like(plain)
    assert qnet.flatten(p, buf) is buf and torch.equal(buf, plain)
    with pytest.raises(ValueError, match="plain buffer"):
        qnet.flatten(p, torch.zeros(plain.numel() + 1))


def test_qnet_entry_points_validate_without_device():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    L = _lib.lib()

    def fragments(chunk, ff, layers):       # 1 KiB each: conv2 4 row tiles, embedding 8, per layer V 8, out_proj 8, linear1 ff / 16, linear2 8; fc 1
        return 4 * (128 // chunk) + 8 * (1024 // chunk) + layers * (16 * (128 // chunk) + (ff // 16) * (128 // chunk) + 8 * (ff // chunk)) + 128 // chunk

    def f32_section(ff, layers):            # conv1 160, conv2 bias 64, embedding bias 128 | per layer 3 x 128 + ff + 512 + 4 | fc bias 16
        return 4 * (352 + layers * (900 + ff) + 16)

    for ff, layers in ((2048, 2), (64, 2), (32, 1), (96, 3)):
        f32, bf16 = L.g2048_qnet_packed_bytes(0, ff, layers), L.g2048_qnet_packed_bytes(1, ff, layers)
        assert f32 == 1024 * fragments(16, ff, layers) + f32_section(ff, layers) and f32 % 16 == 0
        assert bf16 == 1024 * fragments(32, ff, layers) + f32_section(ff, layers) and bf16 % 16 == 0
    # every weight the forward reads, once: the V third of in_proj only, fc padded to one row tile
    assert L.g2048_qnet_packed_bytes(0, 2048, 2) == 4 * (8192 + 131072 + 2 * (2 * 16384 + 2 * 128 * 2048) + 16 * 128) + f32_section(2048, 2)
    for bad in ((2, 64, 2), (-1, 64, 2), (0, 48, 2), (0, 0, 2), (0, 64, 0), (0, -32, 1)):
        assert L.g2048_qnet_packed_bytes(*bad) == 0, bad
    buf = (C.c_uint8 * 256)()
    a = (C.addressof(buf) + 15) & ~15
    assert L.g2048_qnet_forward(None, None, None, None, 0, 64, 2, 0, None) == 0               # n == 0: nothing to do
    assert L.g2048_qnet_forward(None, a, a, None, 8, 64, 2, 0, None) == -1 and b"null pointer" in L.g2048_last_error()
    assert L.g2048_qnet_forward(a, None, a, None, 8, 64, 2, 0, None) == -1 and b"null pointer" in L.g2048_last_error()
    assert L.g2048_qnet_forward(a, a, None, a, 8, 64, 2, 0, None) == -1 and b"null pointer" in L.g2048_last_error()
    assert L.g2048_qnet_forward(a + 4, a, a, None, 8, 64, 2, 0, None) == -1 and b"misaligned" in L.g2048_last_error()
    assert L.g2048_qnet_forward(a, a + 8, a, None, 8, 64, 2, 0, None) == -1 and b"misaligned" in L.g2048_last_error()
    assert L.g2048_qnet_forward(a, a, a + 4, None, 8, 64, 2, 0, None) == -1 and b"misaligned" in L.g2048_last_error()
    assert L.g2048_qnet_forward(a, a, a, None, 8, 64, 2, 2, None) == -1 and b"opts" in L.g2048_last_error()
    assert L.g2048_qnet_forward(a, a, a, None, 8, 48, 2, 0, None) == -1 and b"dim_ff" in L.g2048_last_error()
    assert L.g2048_qnet_forward(a, a, a, None, 8, 64, 0, 0, None) == -1 and b"n_layers" in L.g2048_last_error()
    assert L.g2048_qnet_pack(None, 64, 2, 0, a, None) == -1 and b"null pointer" in L.g2048_last_error()
    assert L.g2048_qnet_pack(a, 64, 2, 7, a, None) == -1 and b"precision" in L.g2048_last_error()
    assert L.g2048_qnet_pack(a, 48, 2, 0, a, None) == -1 and b"dim_ff" in L.g2048_last_error()
    assert L.g2048_qnet_pack(a, 64, 2, 0, a + 8, None) == -1 and b"misaligned" in L.g2048_last_error()
