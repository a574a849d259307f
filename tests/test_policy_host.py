"""CPU-side checks of g2048.DevicePolicy's converter: which modules it accepts, the f64 BatchNorm fold against torch's own eval
forward, the reference's batch-of-one rule, the trained checkpoint of tests/golden/policy.npz, and the C-ABI's argument
validation. The kernel itself is checked on the GPU (tests/test_gpu_policy.py)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import load_golden


class RefLayout(nn.Module):
    """The reference's ActorNetwork / CriticNetwork layout (agents/ppo_agent.py:61-136): fc1..fc4, bn1 / bn2 applied after the
    ReLU and only for batches of more than one row, dropout, softmax for the actor."""

    def __init__(self, n_out=4):
        super().__init__()
        self.fc1, self.bn1 = nn.Linear(16, 256), nn.BatchNorm1d(256)
        self.fc2, self.bn2 = nn.Linear(256, 128), nn.BatchNorm1d(128)
        self.fc3, self.fc4 = nn.Linear(128, 64), nn.Linear(64, n_out)
        self.relu, self.dropout = nn.ReLU(), nn.Dropout(0.2)
        self.softmax = nn.Softmax(dim=-1) if n_out == 4 else None

    def forward(self, x):
        single = x.dim() == 1
        if single:
            x = x.unsqueeze(0)
        x = self.relu(self.fc1(x))
        if x.shape[0] > 1:
            x = self.bn1(x)
        x = self.dropout(x)
        x = self.relu(self.fc2(x))
        if x.shape[0] > 1:
            x = self.bn2(x)
        x = self.dropout(x)
        x = self.fc4(self.relu(self.fc3(x)))
        if self.softmax is not None:
            x = self.softmax(x)
        return x.squeeze(0) if single else x


def bench_trunk_net(n_out):
    """bench.py's ActorCritic halves: nested Sequential, Linear -> BatchNorm -> ReLU, no softmax at the end."""
    def trunk():
        return nn.Sequential(nn.Linear(16, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Linear(256, 128), nn.BatchNorm1d(128),
                             nn.ReLU(), nn.Linear(128, 64), nn.BatchNorm1d(64), nn.ReLU())
    return nn.Sequential(trunk(), nn.Linear(64, n_out))


def perturb_bn(module, gen):
    """Non-trivial running statistics / affine parameters so that a wrong fold shows."""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 1.5 + 0.25)
                m.weight.copy_(1 + 0.3 * torch.randn(m.num_features, generator=gen))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=gen))
    return module.eval()


def random_boards(n, seed=0):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 12, size=(n, 16)).astype(np.uint8)
    b[rng.random((n, 16)) < 0.35] = 0
    b[:4, :] = 0                                 # empty boards
    b[4, :] = 17                                 # the largest code (x = 17 / 15 > 1)
    return b


def distinct_layers(layers, seed):
    """nn.TransformerEncoder deep-copies one layer, so the layers of a fresh module carry the SAME weights (and zero attention
    biases): a kernel that read layer 1's weights for layer 2 would compute the same thing. Adds to every parameter of every given
    layer its own uniform draws from (-0.05, 0.05), in place, so that each layer's tensors are its own and no bias is zero."""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in layers:
            for p in layer.parameters():
                p.add_(((torch.rand(p.shape, generator=g, dtype=torch.float64) - 0.5) * 0.1).to(p.dtype))
    return layers


def numpy_forward(sd, x, batchnorm, softmax):
    """f64 NumPy forward of the reference layout straight from a state dict (no folding): the independent yardstick."""
    g = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    h = np.asarray(x, dtype=np.float64)

    def bn(h, name):
        return (h - g[name + ".running_mean"]) / np.sqrt(g[name + ".running_var"] + 1e-5) * g[name + ".weight"] + g[name + ".bias"]
    h = np.maximum(h @ g["fc1.weight"].T + g["fc1.bias"], 0)
    if batchnorm:
        h = bn(h, "bn1")
    h = np.maximum(h @ g["fc2.weight"].T + g["fc2.bias"], 0)
    if batchnorm:
        h = bn(h, "bn2")
    h = np.maximum(h @ g["fc3.weight"].T + g["fc3.bias"], 0)
    z = h @ g["fc4.weight"].T + g["fc4.bias"]
    if softmax:
        z = np.exp(z - z.max(1, keepdims=True))
        z = z / z.sum(1, keepdims=True)
    return z


def state_dict_np(module):
    return {k: v.detach().cpu().numpy() for k, v in module.state_dict().items() if not k.endswith("num_batches_tracked")}


def golden_modules():
    g = load_golden("policy.npz")
    actor, critic = RefLayout(4), RefLayout(1)
    for prefix, m in (("actor.", actor), ("critic.", critic)):
        sd = {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
        m.eval()
    return g, actor, critic


def fold_forward(module, n_out, x, apply_bn):
    from g2048 import policy
    layers, _ = policy.parse(module, n_out)
    return policy.forward_reference(policy.fold(layers, apply_bn), torch.as_tensor(x), softmax=n_out == 4).numpy()


def _close(got, want, kind):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()
    bound = 1e-6 if kind == "probs" else 1e-5 * np.abs(want).max()
    assert err <= bound, "%s: max error %.3g > %.3g" % (kind, err, bound)


@pytest.mark.parametrize("layout", ["reference", "sequential_bn_after_linear", "sequential_bn_after_relu"])
def test_fold_reproduces_torch_eval_forward(layout):
    gen = torch.Generator().manual_seed(11)
    torch.manual_seed(11)
    if layout == "reference":
        actor, critic = RefLayout(4), RefLayout(1)
    elif layout == "sequential_bn_after_linear":
        actor, critic = bench_trunk_net(4), bench_trunk_net(1)
    else:                                        # the reference's order spelt as a Sequential, with dropout and a softmax
        def net(n_out):
            tail = [nn.Linear(64, n_out)] + ([nn.Softmax(dim=-1)] if n_out == 4 else [])
            return nn.Sequential(nn.Linear(16, 256), nn.ReLU(), nn.BatchNorm1d(256), nn.Dropout(0.2), nn.Linear(256, 128), nn.ReLU(),
                                 nn.BatchNorm1d(128), nn.Dropout(0.2), nn.Linear(128, 64), nn.ReLU(), *tail)
        actor, critic = net(4), net(1)
    perturb_bn(actor, gen)
    perturb_bn(critic, gen)
    x = torch.from_numpy(random_boards(1024, 3).astype(np.float32) / np.float32(15))
    with torch.no_grad():
        pa, va = actor(x), critic(x)
    if layout == "sequential_bn_after_linear":
        pa = torch.softmax(pa, -1)
    _close(fold_forward(actor, 4, x, True), pa.numpy(), "probs")
    _close(fold_forward(critic, 1, x, True), va.numpy(), "values")


def test_batch_of_one_skips_batchnorm_in_the_reference_layout():
    from g2048 import policy
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(5)
    actor, critic = perturb_bn(RefLayout(4), gen), perturb_bn(RefLayout(1), gen)
    x = torch.from_numpy(random_boards(16, 4).astype(np.float32) / np.float32(15))
    with torch.no_grad():
        one_a = torch.stack([actor(x[i]) for i in range(16)])
        one_c = torch.stack([critic(x[i]) for i in range(16)])
    _close(fold_forward(actor, 4, x, False), one_a.numpy(), "probs")
    _close(fold_forward(critic, 1, x, False), one_c.numpy(), "values")
    # ... and the BatchNorm really matters here, so the rule is observable
    assert np.abs(fold_forward(actor, 4, x, True) - one_a.numpy()).max() > 1e-3
    assert policy.parse(actor, 4)[1] is True and policy.parse(bench_trunk_net(4).eval(), 4)[1] is False


def test_golden_checkpoint_through_the_converter():
    g, actor, critic = golden_modules()
    x = g["boards"].astype(np.float32) / np.float32(15)
    _close(fold_forward(actor, 4, x, True), g["probs_batched"], "probs")
    _close(fold_forward(critic, 1, x, True), g["values_batched"], "values")
    k = g["probs_single"].shape[0]
    _close(fold_forward(actor, 4, x[:k], False), g["probs_single"], "probs")
    _close(fold_forward(critic, 1, x[:k], False), g["values_single"], "values")
    # the independent NumPy forward agrees with the recorded reference outputs too
    sd = state_dict_np(actor)
    _close(numpy_forward(sd, x, True, True), g["probs_batched"], "probs")


def test_converter_rejects_what_it_cannot_run():
    from g2048 import policy
    ok = bench_trunk_net(4).eval()
    policy.parse(ok, 4)
    with pytest.raises(ValueError, match="training mode"):
        policy.parse(bench_trunk_net(4), 4)                   # a fresh module is in training mode
    with pytest.raises(ValueError, match="training mode"):
        policy.parse(RefLayout(4), 4)
    with pytest.raises(ValueError, match="expected 16->256"):
        policy.parse(nn.Sequential(nn.Linear(8, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(), nn.Linear(128, 64), nn.ReLU(),
                                   nn.Linear(64, 4)).eval(), 4)
    with pytest.raises(ValueError, match="expected 64->1"):
        policy.parse(ok, 1)                                    # actor-sized head given as a critic
    wide = RefLayout(4)
    wide.fc3 = nn.Linear(128, 32)
    with pytest.raises(ValueError):
        policy.parse(wide.eval(), 4)
    with pytest.raises(ValueError, match="unsupported layer Tanh"):
        policy.parse(nn.Sequential(nn.Linear(16, 256), nn.Tanh(), nn.Linear(256, 128), nn.ReLU(), nn.Linear(128, 64), nn.ReLU(),
                                   nn.Linear(64, 4)).eval(), 4)
    with pytest.raises(ValueError, match="ReLU"):
        policy.parse(nn.Sequential(nn.Linear(16, 256), nn.Linear(256, 128), nn.ReLU(), nn.Linear(128, 64), nn.ReLU(),
                                   nn.Linear(64, 4)).eval(), 4)
    with pytest.raises(ValueError, match="Softmax"):
        policy.parse(nn.Sequential(nn.Linear(16, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(), nn.Linear(128, 64), nn.ReLU(),
                                   nn.Linear(64, 1), nn.Softmax(dim=-1)).eval(), 1)
    with pytest.raises(ValueError, match="neither"):
        policy.parse(nn.Linear(16, 4).eval(), 4)
    nostats = bench_trunk_net(4)
    nostats[0][1] = nn.BatchNorm1d(256, track_running_stats=False)
    with pytest.raises(ValueError, match="running statistics"):
        policy.parse(nostats.eval(), 4)
    from g2048 import DevicePolicy
    with pytest.raises(ValueError, match="precision"):
        DevicePolicy(ok, precision="f16")
    with pytest.raises(ValueError, match="batchnorm"):
        DevicePolicy(ok, batchnorm="sometimes")
    with pytest.raises(RuntimeError, match="no CPU path"):
        DevicePolicy(ok)                                       # the modules live on the CPU


def test_policy_entry_points_validate_without_device():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    L = _lib.lib()
    assert L.g2048_policy_packed_bytes(0, 4) == L.g2048_policy_packed_bytes(0, 1) > 0
    assert 0 < L.g2048_policy_packed_bytes(1, 4) < L.g2048_policy_packed_bytes(0, 4)
    assert L.g2048_policy_packed_bytes(2, 4) == 0 and L.g2048_policy_packed_bytes(0, 3) == 0
    assert L.g2048_policy_packed_bytes(0, 4) % 16 == 0 and L.g2048_policy_packed_bytes(1, 4) % 16 == 0
    buf = (C.c_uint8 * 256)()
    a = (C.addressof(buf) + 15) & ~15
    assert L.g2048_policy_forward(None, None, None, None, None, 0, 0, None) == 0          # n == 0: nothing to do
    assert L.g2048_policy_forward(None, a, None, a, None, 8, 0, None) == -1 and b"null pointer" in L.g2048_last_error()
    assert L.g2048_policy_forward(a, a, a, a, None, 8, 0, None) == -1 and b"both" in L.g2048_last_error()
    assert L.g2048_policy_forward(a + 4, a, None, a, None, 8, 0, None) == -1 and b"misaligned" in L.g2048_last_error()
    assert L.g2048_policy_forward(a, a, a, a, a + 2, 8, 0, None) == -1 and b"misaligned" in L.g2048_last_error()
    assert L.g2048_policy_forward(a, a, None, a, None, 8, 2, None) == -1 and b"opts" in L.g2048_last_error()
    assert L.g2048_policy_pack(None, 4, 0, a, None) == -1 and b"null pointer" in L.g2048_last_error()
    assert L.g2048_policy_pack(a, 2, 0, a, None) == -1 and b"n_out" in L.g2048_last_error()
    assert L.g2048_policy_pack(a, 4, 7, a, None) == -1 and b"precision" in L.g2048_last_error()
    assert L.g2048_policy_pack(a, 4, 0, a + 8, None) == -1 and b"misaligned" in L.g2048_last_error()
