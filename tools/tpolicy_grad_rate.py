"""DeviceTransformerPolicy.loss_and_grad (PPOAgent.update()'s loss on the transformer policy's two heads and its gradient,
g2048_tpolicy_loss_grad) against stock torch on the same GPU.

    python3 tools/tpolicy_grad_rate.py                    the table
    python3 tools/tpolicy_grad_rate.py --dropout          what the encoder's live dropout costs (the training library)
    python3 tools/tpolicy_grad_rate.py --grad-precision bf16   the f32 pass and the bf16 feed-forward mode side by side, at dropout 0
                                                          and 0.1 (profiles/r37_tpolicy_bf16_rate.txt keeps a run)

The reference's layout (torch's default init, the heads x 8) with dim_ff 128 (bench.py's config 4) and 2,048 (the reference's), 2
layers, at N = 64, 256 and 1,024 boards. Versions, alternating within every round:
  torch f32 fwd+bwd     the stock eval-mode module's own forward, the same loss with torch.distributions.Categorical,
                        zero_grad(set_to_none=False) and backward(): the yardstick (eval mode on both sides: no dropout);
  device loss_and_grad  the same function: the forward with its activations kept, the loss head and the backward.
A round times REPS back-to-back calls of a version between one event pair and divides; median of 7 rounds after 2 warm-up rounds,
min - max in brackets. Before timing, the device gradients and stock torch's float32 ones are both compared with the module's
float64 autograd on the same GPU, per tensor as max|g - g64| / max|g64|. The boards are not screened: where a ReLU input lies within
rounding of zero, either side's gradient shows a sign flip (1e-4 .. 1e-3); tests/tpolicy_grad_ref.py screens its cases for that.
Output: one text table (profiles/r29_tpolicy_grad_rate.txt keeps a run).

--dropout: at N = 256 and 1,024, dim_ff 128 and 2,048, 2 layers, alternating within every round: the learner library's
g2048_tpolicy_loss_grad; the training library's g2048_tpolicy_loss_grad_dropout at p = 0 (the same kernels in the same order: it must
lie inside the first row's spread), at p = 0.1 on all four sites and on each site alone; the stock module in .train() mode (forward,
loss, backward()) at p = 0 and p = 0.1 with torch's own masks; net.update(epochs=8) at p = 0 and p = 0.1
(profiles/r32_tpolicy_dropout_rate.txt keeps a run)."""
import copy
import ctypes as C
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import DeviceTransformerPolicy, ops  # noqa: E402
from g2048 import _lib as L  # noqa: E402

dev = torch.device("cuda")
LAYERS, REPS = 2, 10
CLIP, VALUE_COEF, ENTROPY_COEF = 0.3, 0.4, 0.05


class TPolicy(nn.Module):               # the reference's structure and forward, stock torch, default init
    def __init__(self, dim_ff, layers=LAYERS):
        super().__init__()
        self.embedding = nn.Linear(1, 64)
        layer = nn.TransformerEncoderLayer(d_model=64, nhead=4, dim_feedforward=dim_ff, batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=layers, enable_nested_tensor=False)
        self.fc1, self.fc2 = nn.Linear(1024, 128), nn.Linear(128, 64)
        self.actor, self.critic = nn.Linear(64, 4), nn.Linear(64, 1)

    def forward(self, x):
        n = x.size(0)
        x = self.transformer_encoder(self.embedding(x.view(n, 16, 1))).reshape(n, -1)
        x = torch.relu(self.fc2(torch.relu(self.fc1(x))))
        return torch.softmax(self.actor(x), dim=-1), self.critic(x)


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / REPS


def alternate(versions, warmup=2, rounds=7):
    times = {name: [] for name, _ in versions}
    for r in range(warmup + rounds):
        for name, fn in versions:
            dt = event_time(fn)
            if r >= warmup:
                times[name].append(dt)
    return times


def stock_loss(model, x, actions, old, adv, ret):
    probs, value = model(x)
    dist = torch.distributions.Categorical(probs=probs)
    ratio = torch.exp(dist.log_prob(actions) - old)
    actor = -torch.min(ratio * adv, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * adv).mean()
    return actor + VALUE_COEF * ((value[:, 0] - ret) ** 2).mean() - ENTROPY_COEF * dist.entropy().mean()


def grads_of(model, x, actions, old, adv, ret):
    dtype = next(model.parameters()).dtype
    model.zero_grad(set_to_none=False)
    stock_loss(model, x.to(dtype), actions, old.to(dtype), adv.to(dtype), ret.to(dtype)).backward()
    return [p.grad.detach().double().reshape(-1).clone() for p in model.parameters()]


def main():
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    print("%-8s %-6s %-24s %-24s %-9s %s" % ("dim_ff", "N", "torch f32 fwd+bwd", "device loss_and_grad", "speed-up", "error vs f64: device, torch f32"))
    for dim_ff in (128, 2048):
        torch.manual_seed(29)
        model = TPolicy(dim_ff).to(dev).eval()
        with torch.no_grad():
            model.actor.weight.mul_(8.0)
            model.critic.weight.mul_(8.0)
        model64 = copy.deepcopy(model).double()
        net = DeviceTransformerPolicy(copy.deepcopy(model))
        for n in (64, 256, 1024):
            boards = ops.synth_boards(n, seed=29 + n, device=dev)
            x = boards.float() / 15
            i = torch.arange(n, device=dev)
            actions = (5 * i + 1) % 4
            gen = torch.Generator(device=dev).manual_seed(n)
            with torch.no_grad():
                p64, v64 = model64(x.double())
            old = (torch.log(p64.gather(1, actions[:, None])[:, 0]) + 0.5 * torch.randn(n, generator=gen, device=dev, dtype=torch.float64)).float()
            adv = (((13 * i) % 17 - 8) / 4.0 + 2.0 * x[:, 0]).float()
            ret = (v64[:, 0] + 0.5 + ((7 * i) % 11 - 5) / 5.0).float()
            g64 = grads_of(model64, x, actions, old, adv, ret)
            g32 = grads_of(model, x, actions, old, adv, ret)
            net.loss_and_grad(boards, actions, old, adv, ret)
            flat, o, gdev = net.grad.double(), 0, []
            for t in net.parsed.plain_tensors():
                k = t.numel() if isinstance(t, torch.Tensor) else 1
                if isinstance(t, torch.Tensor):
                    gdev.append(flat[o:o + k])
                o += k
            err = lambda gs: max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gs, g64))      # noqa: E731

            def stock():
                model.zero_grad(set_to_none=False)
                stock_loss(model, x, actions, old, adv, ret).backward()

            t = alternate([("torch", stock), ("device", lambda: net.loss_and_grad(boards, actions, old, adv, ret))])
            cell = lambda v: "%8.1f us [%7.1f - %7.1f]" % (statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6)      # noqa: E731
            print("%-8d %-6d %-24s %-24s %-9s %.2g, %.2g" % (dim_ff, n, cell(t["torch"]), cell(t["device"]),
                                                            "%.2f x" % (statistics.median(t["torch"]) / statistics.median(t["device"])),
                                                            err(gdev), err(g32)))
        print("workspace at N = 1,024, dim_ff %d, 2 layers: %.1f MiB" % (dim_ff, ops.tpolicy_grad_workspace_bytes(1024, dim_ff, LAYERS) / 2 ** 20))


def dropout_table():
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    sites = ("attention", "dropout1", "dropout", "dropout2")
    for dim_ff in (128, 2048):
        torch.manual_seed(29)
        model = TPolicy(dim_ff).to(dev).eval()
        with torch.no_grad():
            model.actor.weight.mul_(8.0)
            model.critic.weight.mul_(8.0)
        plain = DeviceTransformerPolicy(copy.deepcopy(model))
        dropped = DeviceTransformerPolicy(copy.deepcopy(model), dropout=0.1)
        trains = {}
        for p in (0.0, 0.1):
            trains[p] = copy.deepcopy(model).train()
            for lay in trains[p].transformer_encoder.layers:
                lay.self_attn.dropout, lay.dropout1.p, lay.dropout.p, lay.dropout2.p = p, p, p, p
        for n in (256, 1024):
            boards, nxt = ops.synth_boards(n, seed=29 + n, device=dev), ops.synth_boards(n, seed=59 + n, device=dev)
            x = boards.float() / 15
            i = torch.arange(n, device=dev)
            actions = (5 * i + 1) % 4
            gen = torch.Generator(device=dev).manual_seed(n)
            with torch.no_grad():
                p32, v32 = model(x)
            old = torch.log(p32.gather(1, actions[:, None])[:, 0]) + 0.5 * torch.randn(n, generator=gen, device=dev)
            adv = (((13 * i) % 17 - 8) / 4.0 + 2.0 * x[:, 0]).float()
            ret = (v32[:, 0] + 0.5 + ((7 * i) % 11 - 5) / 5.0).float()
            rewards, dones = ret * 0.5, (i % 5 == 0).float()
            grad = torch.empty_like(plain.plain)
            ws = torch.empty(ops.tpolicy_train_workspace_bytes(n, dim_ff, LAYERS), dtype=torch.uint8, device=dev)
            counter = [0]

            def device(p4):
                def run():
                    counter[0] += 1
                    ops.tpolicy_loss_grad(boards, plain.plain, actions, old, adv, ret, dim_ff, LAYERS, grad=grad, workspace=ws, dropout=p4,
                                          seed=1, call_index=counter[0])
                return run

            out = (torch.empty(4, device=dev), torch.empty((n, 4), device=dev), torch.empty((n, 1), device=dev))
            f, zeros = C.c_float, (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)

            def zero_p():       # the training library's entry point itself at p = 0 (ops would take the learner library's)
                L.ttrain_call(dev, L.ttrain_lib().g2048_tpolicy_loss_grad_dropout, boards.data_ptr(), plain.plain.data_ptr(), actions.data_ptr(),
                              old.data_ptr(), adv.data_ptr(), ret.data_ptr(), n, dim_ff, LAYERS, zeros, 1, 1, f(CLIP),
                              f(VALUE_COEF), f(ENTROPY_COEF), grad.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                              ws.data_ptr(), ws.numel(), L.stream_ptr(dev))

            def stock(p):
                def run():
                    trains[p].zero_grad(set_to_none=False)
                    stock_loss(trains[p], x, actions, old, adv, ret).backward()
                return run

            def update(net):
                return lambda: net.update(boards, actions, old, rewards, nxt, dones, epochs=8)

            versions = [("learner library, eval mode", device(None)), ("training library, p = 0", zero_p),
                        ("training library, p = 0.1 on all four", device(0.1))]
            versions += [("  p = 0.1 on site %d (%s) alone" % (k, sites[k]), device(tuple(0.1 if j == k else 0.0 for j in range(4)))) for k in range(4)]
            versions += [("torch .train() fwd+bwd, p = 0", stock(0.0)), ("torch .train() fwd+bwd, p = 0.1", stock(0.1)),
                         ("update(epochs=8), p = 0", update(plain)), ("update(epochs=8), p = 0.1", update(dropped))]
            start = [plain.plain.clone(), dropped.plain.clone()]
            t = alternate(versions)
            for net, t0 in zip((plain, dropped), start):       # the timed updates moved the weights
                net.plain.copy_(t0)
                net._plain_changed()
            base = statistics.median(t[versions[0][0]])
            print("dim_ff %d, N = %d" % (dim_ff, n))
            for name, _ in versions:
                v = t[name]
                print("  %-42s %9.1f us [%8.1f - %8.1f]  %5.2f x the first row" % (name, statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6,
                                                                                   statistics.median(v) / base))


def precision_table():
    """--grad-precision bf16: the f32 pass and the bf16 feed-forward mode (g2048_tpolicy_loss_grad_bf16) in the same run, each at dropout
    0 and 0.1, alternating within every round; and how far the bf16 mode's gradients lie from the f32 pass's."""
    print("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    print("%-7s %-5s %-30s %-30s %-8s %-30s %-30s %-8s %s" % ("dim_ff", "N", "f32, p = 0", "bf16, p = 0", "f32/bf16", "f32, p = 0.1", "bf16, p = 0.1",
                                                             "f32/bf16", "bf16 against f32 gradients (p = 0)"))
    for dim_ff in (128, 2048):
        torch.manual_seed(29)
        model = TPolicy(dim_ff).to(dev).eval()
        with torch.no_grad():
            model.actor.weight.mul_(8.0)
            model.critic.weight.mul_(8.0)
        nets = {(gp, p): DeviceTransformerPolicy(copy.deepcopy(model), dropout=p, grad_precision=gp) for gp in ("f32", "bf16") for p in (0.0, 0.1)}
        for n in (64, 256, 1024):
            boards = ops.synth_boards(n, seed=29 + n, device=dev)
            x = boards.float() / 15
            i = torch.arange(n, device=dev)
            actions = (5 * i + 1) % 4
            gen = torch.Generator(device=dev).manual_seed(n)
            with torch.no_grad():
                p32, v32 = model(x)
            old = torch.log(p32.gather(1, actions[:, None])[:, 0]) + 0.5 * torch.randn(n, generator=gen, device=dev)
            adv = (((13 * i) % 17 - 8) / 4.0 + 2.0 * x[:, 0]).float()
            ret = (v32[:, 0] + 0.5 + ((7 * i) % 11 - 5) / 5.0).float()
            grads = {}
            for gp in ("f32", "bf16"):
                nets[gp, 0.0].loss_and_grad(boards, actions, old, adv, ret)
                flat, o, grads[gp] = nets[gp, 0.0].grad.double(), 0, []
                for t in nets[gp, 0.0].parsed.plain_tensors():
                    k = t.numel() if isinstance(t, torch.Tensor) else 1
                    if isinstance(t, torch.Tensor):
                        grads[gp].append(flat[o:o + k])
                    o += k
            away = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads["bf16"], grads["f32"]))
            names = [(gp, p) for p in (0.0, 0.1) for gp in ("f32", "bf16")]
            t = alternate([(key, (lambda net: lambda: net.loss_and_grad(boards, actions, old, adv, ret))(nets[key])) for key in names])
            cell = lambda v: "%8.1f us [%7.1f - %7.1f]" % (statistics.median(v) * 1e6, min(v) * 1e6, max(v) * 1e6)      # noqa: E731
            gain = lambda p: "%.2f x" % (statistics.median(t["f32", p]) / statistics.median(t["bf16", p]))             # noqa: E731
            print("%-7d %-5d %-30s %-30s %-8s %-30s %-30s %-8s %.3g of the largest element" % (
                dim_ff, n, cell(t["f32", 0.0]), cell(t["bf16", 0.0]), gain(0.0), cell(t["f32", 0.1]), cell(t["bf16", 0.1]), gain(0.1), away))
        print("workspace at N = 1,024, dim_ff %d, 2 layers: f32 %.1f MiB, f32 with dropout %.1f MiB, bf16 %.1f MiB" % (
            dim_ff, ops.tpolicy_grad_workspace_bytes(1024, dim_ff, LAYERS) / 2 ** 20, ops.tpolicy_train_workspace_bytes(1024, dim_ff, LAYERS) / 2 ** 20,
            ops.tpolicy_bf16_workspace_bytes(1024, dim_ff, LAYERS) / 2 ** 20))


if __name__ == "__main__":
    if sys.argv[1:] == ["--grad-precision", "bf16"]:
        precision_table()
    else:
        dropout_table() if sys.argv[1:] == ["--dropout"] else main()
