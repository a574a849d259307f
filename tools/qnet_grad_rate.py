"""DeviceQNetwork.loss_and_grad (the gradient half of DQNAgent.train_step, agents/hybrid.py:1038 and :1049-1055) against stock
torch on the same GPU.

    python3 tools/qnet_grad_rate.py                       the table
    python3 tools/qnet_grad_rate.py --trace N [CALLS]     only CALLS (50) loss_and_grad calls at n = N, for a kernel trace:
        rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/qnet_grad_rate.py --trace 256
        python3 tools/qnet_grad_rate.py --phases OUT      that trace as one line per phase (the kernels in launch order)
    python3 tools/qnet_grad_rate.py --dropout             what the training library's live dropout costs (dropout_table below;
                                                          profiles/r28_qnet_dropout_rate.txt keeps a run)

The reference's shape (dim_ff 2048, 2 layers, torch's default init) at n = 64, 256 and 1,024 boards; 256 is the batch train_step
uses. Versions, alternating within every round:
  torch f32 fwd+bwd     the stock eval-mode module's own batch call, nn.SmoothL1Loss(reduction='none'), (weights * td).mean(),
                        zero_grad(set_to_none=False) and backward(): the yardstick (eval mode on both sides: no dropout);
  device loss_and_grad  the same function: the forward with its activations kept, the loss and the backward, 50 launches;
  device forward_batch  the forward alone, for context.
A round times REPS back-to-back calls of a version between one event pair and divides; median of 7 rounds after 2 warm-up rounds,
min - max in brackets. Before timing, the device gradients and stock torch's float32 ones are both compared with the module's
float64 autograd on the same GPU, per tensor as max|g - g64| / max|g64|, over the parameters downstream of layer 0's softmax (the
others are no float32 quantity on boards with large tiles: DESIGN.md).
Output: one text table (profiles/r18_qnet_grad_rate.txt keeps a run)."""
import copy
import csv
import glob
import os
import statistics
import sys
from collections import defaultdict

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = [("qb_conv", "forward conv"), ("qb_linear", "forward linear (embedding, in_proj, linear1)"), ("qb_attention", "forward attention"),
          ("qb_proj_norm", "forward out_proj+norm1, linear2+norm2(+fc)"), ("qg_head", "head"), ("qg_sum", "loss sum"),
          ("qg_ln", "LayerNorm backward"), ("qg_tiles", "LayerNorm dgamma / dbeta over the tiles"), ("qg_dx", "data-gradient products"),
          ("qg_dw", "weight-gradient products"), ("qg_att_dq", "attention backward dQ"), ("qg_att_dkv", "attention backward dK, dV"),
          ("qg_conv_dw2", "conv2 weight gradient"), ("qg_conv_dz1", "conv2 transposed into conv1's output"),
          ("qg_conv_dw1", "conv1 weight gradient")]


def phases(directory):
    """One line per kernel and launch size of a rocprofv3 --kernel-trace csv: launches per call, median and minimum duration."""
    for f in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        by = defaultdict(list)
        for row in csv.DictReader(open(f)):
            grid = "x".join(row.get(k, "") for k in ("Grid_Size_X", "Grid_Size_Y") if row.get(k)) or row.get("Grid_Size", "")
            by[(row.get("Kernel_Name", ""), grid)].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        total, calls = 0.0, max([len(v) for (name, _), v in by.items() if "qb_conv_kernel" in name] or [1])
        for key, label in PHASES:
            for (name, grid), v in sorted(by.items()):
                if key + "_kernel" not in name:
                    continue
                v.sort()
                med = v[len(v) // 2] * 1e-3
                total += med * len(v)
                print("%-52s grid %-10s launches %5d   %8.1f us [%8.1f]" % (label, grid, len(v), med, v[0] * 1e-3))
        print("sum of the kernel medians over a call's launches (%d calls traced): %.1f us a call" % (calls, total / calls))


if sys.argv[1:2] == ["--phases"]:
    phases(sys.argv[2])
    sys.exit(0)

import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import DeviceQNetwork, ops  # noqa: E402

dev = torch.device("cuda")
DIM_FF, LAYERS, REPS, N_UPSTREAM = 2048, 2, 10, 8


class QNet(nn.Module):                  # the reference's structure and forward, stock torch, default init
    def __init__(self, dim_ff=DIM_FF, layers=LAYERS):
        super().__init__()
        self.cnn = nn.Sequential(nn.Conv2d(1, 32, kernel_size=2, stride=1, padding=1), nn.ReLU(),
                                 nn.Conv2d(32, 64, kernel_size=2, stride=1, padding=0), nn.ReLU())
        self.embedding = nn.Linear(1024, 128)
        self.transformer = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=128, nhead=8, dim_feedforward=dim_ff), layers,
                                                 enable_nested_tensor=False)
        self.fc = nn.Linear(128, 4)

    def forward(self, x):               # one sequence of B tokens
        h = self.embedding(self.cnn(x.view(-1, 1, 4, 4)).view(x.shape[0], -1))
        return self.fc(self.transformer(h.unsqueeze(1)).squeeze(1))


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / REPS


def alternate(versions, warmup, rounds):
    """{name: [seconds per call and round]}: every round runs each version, in order."""
    times = {name: [] for name, _ in versions}
    for r in range(warmup + rounds):
        for name, fn in versions:
            dt = event_time(fn)
            if r >= warmup:
                times[name].append(dt)
    return times


def tile_values(boards, dtype=torch.float32):
    return torch.where(boards > 0, torch.ones_like(boards, dtype=torch.int64) << boards.to(torch.int64), 0).to(dtype)


def inputs(model64, boards):
    n = boards.shape[0]
    i = torch.arange(n, device=dev)
    actions = (5 * i + 1) % 4
    with torch.no_grad():
        q = model64(tile_values(boards, torch.float64))
    targets = (q.gather(1, actions.unsqueeze(1)).squeeze(1) + ((37 * i + 11) % 101 - 50) / 25.0).to(torch.float32)
    return actions, targets, (0.25 + ((13 * i) % 16) / 16.0).to(torch.float32)


def torch_step(model, x, actions, targets, weights):
    td = nn.SmoothL1Loss(reduction="none")(model(x).gather(1, actions.unsqueeze(1)).squeeze(1), targets)
    loss = (weights * td).mean()
    model.zero_grad(set_to_none=False)
    loss.backward()
    return loss


torch.manual_seed(0)
model = QNet().to(dev).eval()
net = DeviceQNetwork(model)
model64 = copy.deepcopy(model).double()

def dropout_table():
    """--dropout: what the reference's live dropout costs (docs/LOG.md R28.1). At n = 256 and 4,096, the rows alternating within every
    round, median of 7 rounds after 2 warm-up rounds; per row the device clock (an event pair round REPS calls) and the host clock (the
    time the same REPS calls take to enqueue). Before timing, p = 0 through the training library is checked to give the main library's
    bits."""
    import ctypes as C
    import time

    import g2048
    from g2048 import _lib as L
    p1 = 0.1
    target_model = QNet().to(dev).eval()
    nets = {p: DeviceQNetwork(copy.deepcopy(model), dropout=p, dropout_seed=1) for p in (0.0, p1)}
    targets_of = {p: DeviceQNetwork(copy.deepcopy(target_model), dropout=p, dropout_seed=2) for p in (0.0, p1)}
    for d in (nets, targets_of):
        for v in d.values():
            v.attach_params()
    single = {s: tuple(p1 if k == s else 0.0 for k in range(4)) for s in range(4)}
    train = copy.deepcopy(model).train()
    zeros = (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)

    def set_p(m, p):
        for lay in m.transformer.layers:
            lay.self_attn.dropout, lay.dropout1.p, lay.dropout.p, lay.dropout2.p = p, p, p, p

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        h1 = time.perf_counter()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / REPS, (h1 - h0) / REPS

    print("# --dropout: dim_ff %d, %d layers, p = %g; %d calls per event pair; median of 7 rounds after 2 warm-up rounds, the rows alternating"
          % (DIM_FF, LAYERS, p1, REPS))
    print("%-7s %-56s %10s %22s %10s" % ("boards", "version", "device us", "[min - max] us", "host us"))
    for n in (256, 4096):
        boards = ops.synth_boards(n, seed=3, device=dev)
        nxt = ops.synth_boards(n, seed=4, device=dev)
        x = tile_values(boards)
        a, t, w = inputs(model64, boards)
        shaped, dones = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        net0 = nets[0.0]
        floats = net0.plain.numel()
        grad, td, q, loss = (torch.empty(s, device=dev) for s in ((floats,), (n,), (n, 4), ()))
        ws = torch.empty(ops.qnet_train_workspace_bytes(n, DIM_FF, LAYERS), dtype=torch.uint8, device=dev)

        def main_lib():
            ops.qnet_loss_grad(boards, net0.plain, a, t, w, DIM_FF, LAYERS, grad=grad, td=td, loss=loss, q=q, workspace=ws)

        def train_lib_p0():
            L.train_call(dev, L.train_lib().g2048_qnet_loss_grad_dropout, boards.data_ptr(), net0.plain.data_ptr(), a.data_ptr(), t.data_ptr(),
                         w.data_ptr(), n, DIM_FF, LAYERS, zeros, 1, 2, grad.data_ptr(), td.data_ptr(), loss.data_ptr(), q.data_ptr(),
                         ws.data_ptr(), L.stream_ptr(dev))

        main_lib()
        want = grad.clone()
        train_lib_p0()
        assert torch.equal(grad, want), "p = 0 through the training library does not give the main library's bits"

        def site_row(p4):
            return lambda: ops.qnet_loss_grad(boards, net0.plain, a, t, w, DIM_FF, LAYERS, grad=grad, td=td, loss=loss, q=q, workspace=ws,
                                              dropout=p4, seed=1, call_index=2)

        def torch_row(p):
            def fn():
                set_p(train, p)
                torch_step(train, x, a, t, w)
            return fn

        def round_row(p):
            online, target = nets[p], targets_of[p]

            def fn():
                tg, _ = g2048.dqn_targets(online, target, nxt, shaped, dones, 0.99, training=True)
                online.loss_and_grad(boards, a, tg, w)
                online.adamw_step(1e-4)
            return fn

        rows = ([("main library g2048_qnet_loss_grad", main_lib), ("training library, p = 0", train_lib_p0),
                 ("training library, p = %g on all four sites" % p1, site_row((p1,) * 4))]
                + [("training library, p = %g on site %d (%s) alone" % (p1, s, ops.QNET_DROPOUT_SITES[s]), site_row(single[s])) for s in range(4)]
                + [("torch training-mode fwd+bwd, p = 0", torch_row(0.0)), ("torch training-mode fwd+bwd, p = %g" % p1, torch_row(p1)),
                   ("round: targets + loss_and_grad + adamw_step, p = 0", round_row(0.0)),
                   ("round: targets + loss_and_grad + adamw_step, p = %g" % p1, round_row(p1))])
        times = {name: [] for name, _ in rows}
        for r in range(9):
            for name, fn in rows:
                dt = timed(fn)
                if r >= 2:
                    times[name].append(dt)
        for name, _ in rows:
            devs, hosts = [d for d, _ in times[name]], [h for _, h in times[name]]
            print("%-7d %-56s %10.1f %22s %10.1f" % (n, name, statistics.median(devs) * 1e6, "[%.1f - %.1f]" % (min(devs) * 1e6, max(devs) * 1e6),
                                                    statistics.median(hosts) * 1e6))
        train.zero_grad(set_to_none=True)


if sys.argv[1:2] == ["--dropout"]:
    dropout_table()
    sys.exit(0)

if sys.argv[1:2] == ["--trace"]:
    n, calls = int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 50
    boards = ops.synth_boards(n, seed=3, device=dev)
    a, t, w = inputs(model64, boards)
    for _ in range(calls):
        net.loss_and_grad(boards, a, t, w)
    torch.cuda.synchronize()
    print("%d loss_and_grad calls at n = %d" % (calls, n))
    sys.exit(0)

print("# dim_ff %d, %d layers; %d calls per event pair; median of 7 rounds after 2 warm-up rounds, the versions alternating" % (DIM_FF, LAYERS, REPS))
print("# workspace of loss_and_grad: %s" % ", ".join("n = %d: %.1f MB" % (n, ops.qnet_grad_workspace_bytes(n, DIM_FF, LAYERS) / 1e6) for n in (64, 256, 1024)))
print("%-7s %-22s %10s %22s %12s %10s" % ("boards", "version", "us", "[min - max] us", "boards/s", "vs torch"))
for n in (64, 256, 1024):
    boards = ops.synth_boards(n, seed=3, device=dev)
    x = tile_values(boards)
    a, t, w = inputs(model64, boards)
    torch_step(model64, x.double(), a, t.double(), w.double())
    want = [p.grad.reshape(-1).clone() for p in model64.parameters()]
    torch_step(model, x, a, t, w)
    got32 = [p.grad.reshape(-1).double() for p in model.parameters()]
    net.loss_and_grad(boards, a, t, w)
    o, got = 0, []
    for p in net.parsed.plain_tensors():
        k = p.numel() if isinstance(p, torch.Tensor) else 1
        if isinstance(p, torch.Tensor):
            got.append(net.grad[o:o + k].double())
        o += k
    ratio = lambda gs: [((g - z).abs().max() / z.abs().max()).item() for g, z in zip(gs, want)]
    r_dev, r_torch = ratio(got), ratio(got32)
    print("# n = %d: worst max|g - g64| / max|g64| downstream of the layer-0 softmax: device %.3g, torch f32 %.3g; upstream of it "
          "(no float32 quantity): device %.3g, torch f32 %.3g" % (n, max(r_dev[N_UPSTREAM:]), max(r_torch[N_UPSTREAM:]),
                                                                 max(r_dev[:N_UPSTREAM]), max(r_torch[:N_UPSTREAM])))
    assert max(r_dev[N_UPSTREAM:]) <= 8 * max(r_torch[N_UPSTREAM:]), "loss_and_grad does not compute torch's gradients"
    versions = [("torch f32 fwd+bwd", lambda: torch_step(model, x, a, t, w)), ("device loss_and_grad", lambda: net.loss_and_grad(boards, a, t, w)),
                ("device forward_batch", lambda: net.forward_batch(boards))]
    times = alternate(versions, 2, 7)
    base = statistics.median(times["torch f32 fwd+bwd"])
    for name, _ in versions:
        tt = times[name]
        med = statistics.median(tt)
        print("%-7d %-22s %10.1f %22s %12.4g %9.2fx" % (n, name, med * 1e6, "[%.1f - %.1f]" % (min(tt) * 1e6, max(tt) * 1e6), n / med, base / med))
    model.zero_grad(set_to_none=True)
