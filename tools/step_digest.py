"""The three optimiser-step entry points (g2048_qnet_adamw_step, g2048_tpolicy_adam_step, g2048_ppo_adam_step) from seeded states: one
SHA-256 per case over every buffer, the counters and the norms after two calls. Two builds compute the same bits if and only if
their lists are equal:

    python3 tools/step_digest.py [--out FILE]                                                    the product's libraries
    G2048_LIB=A.so G2048_TSTEP_LIB=B.so python3 tools/step_digest.py [--out FILE]                 another build's
    python3 tools/step_digest.py --compare FILE FILE                                             (host) the cases that differ

Cases. Q-network and transformer policy: dim_ff, n_layers = 32,1 (the eps pair in the first half of a 16-byte group, one tail
length), 32,2 (the second half, the other tail length), 32,3 (both within one buffer), 96,2 (a third dim_ff) and 2048,2 / 4096,2 (the
smallest shapes whose chunk is 2,048 floats: a block makes two passes), each at step 1 and 6 with max_norm None, 0.3 (clipping)
and 10; the Q-network with weight_decay 0 and 1e-4; the policy with no loss tensor, a finite loss, a NaN loss (skipped) and a
gradient that holds one inf (skipped). The PPO pair: its one shape with the same gates, lr and eps as pairs, counters {5, 3, 1, 2}.
Before it prints a digest the tool asserts that the case exercises what it names: at max_norm 0.3 the gradient left behind differs
in bits from the one given, and (1 / (norm + 1e-6)) * max_norm differs from max_norm / (norm + 1e-6) in float32; a skipped call
leaves every buffer as it was."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compare(a, b):
    rows = [dict(line.split() for line in open(f) if line.strip() and not line.startswith("#")) for f in (a, b)]
    differ = sorted(k for k in set(rows[0]) | set(rows[1]) if rows[0].get(k) != rows[1].get(k))
    print("%d cases in %s, %d in %s: %d differ" % (len(rows[0]), a, len(rows[1]), b, len(differ)))
    for k in differ:
        print("  " + k)
    return 1 if differ or not rows[0] else 0


if sys.argv[1:2] == ["--compare"]:
    sys.exit(compare(sys.argv[2], sys.argv[3]))

import torch  # noqa: E402

sys.path.insert(0, REPO)
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import _lib, ops  # noqa: E402

dev = torch.device("cuda")
MAX_NORMS = (None, 0.3, 10.0)
GATES = ("no loss", "finite loss", "nan loss", "inf grad")
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def both_clip_forms_differ(norm):
    """At this float32 norm and at its two neighbours, so that the last bit of the norm does not decide it."""
    f = np.float32
    for n in (norm, np.nextafter(f(norm), f(0)), np.nextafter(f(norm), f(np.inf))):
        d = f(n) + f(1e-6)
        if (f(1.0) / d) * f(0.3) == f(0.3) / d:
            return False
    return True


def state(floats, seed):
    """plain, grad, exp_avg, exp_avg_sq of `floats` floats on the host: the gradient's norm lies between 0.3 and 10, and is scaled
    up in small steps until the two forms of the clip coefficient differ there."""
    g = torch.Generator().manual_seed(seed)
    plain = torch.randn(floats, generator=g) * 0.05
    grad = torch.randn(floats, generator=g) * (1.0 / floats ** 0.5)
    exp_avg = torch.randn(floats, generator=g) * 0.01
    exp_avg_sq = torch.rand(floats, generator=g) * 1e-4
    for k in range(2048):       # one norm in sixty has the property with both its neighbours
        scaled = (grad * (1.0 + k / 1024.0)).float()
        norm = float(scaled.double().square().sum().sqrt().float())
        if both_clip_forms_differ(norm):
            assert 0.3 < norm < 10.0, norm
            return [plain, scaled, exp_avg, exp_avg_sq]
    raise AssertionError("no gradient scale at which the two clip forms differ")


def digest(tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_case(name, before, after, norms, max_norm, skipped):
    """before, after: lists of (plain, grad, exp_avg, exp_avg_sq) per network after the FIRST call; norms: one per network."""
    for net, (b, a) in enumerate(zip(before, after)):
        if skipped:
            assert all(bits_equal(x, y) for x, y in zip(b, a)), "%s: a skipped call wrote a buffer" % name
            continue
        assert not bits_equal(b[0], a[0]), "%s: the weights did not move" % name
        if max_norm == 0.3:
            assert not bits_equal(b[1], a[1]), "%s: the gradient left behind is the one given: nothing was clipped" % name
            assert both_clip_forms_differ(float(norms[net])), "%s: both clip forms agree at norm %r" % (name, float(norms[net]))
        else:
            assert bits_equal(b[1], a[1]), "%s: the gradient was clipped" % name


def run_encoder(kind, dim_ff, layers, host_state):
    for step in (1, 6):
        for max_norm in MAX_NORMS:
            for variant in ((0.0, 1e-4) if kind == "qnet" else GATES):
                bufs = [t.clone().to(dev) for t in host_state]
                name = "%s ff=%d L=%d step=%d max_norm=%s %s" % (kind, dim_ff, layers, step, max_norm,
                                                               "wd=%g" % variant if kind == "qnet" else variant.replace(" ", "_"))
                extra, skipped = [], False
                if kind == "qnet":
                    call = lambda s: ops.qnet_adamw_step(*bufs, dim_ff, layers, 1e-3, s, betas=(0.9, 0.999), eps=1e-8,       # noqa: E731
                                                         weight_decay=variant, max_norm=max_norm)
                else:
                    counters = torch.tensor([step - 1, 2, 1], dtype=torch.int64, device=dev)
                    losses = {"no loss": None, "nan loss": torch.tensor([float("nan"), 0, 0, 0], dtype=torch.float32, device=dev)}.get(
                        variant, torch.tensor([0.75, 0, 0, 0], dtype=torch.float32, device=dev))
                    if variant == "inf grad":
                        bufs[1][bufs[1].numel() // 3] = float("inf")
                    skipped = variant in ("nan loss", "inf grad")
                    extra = [counters]
                    call = lambda s: ops.tpolicy_adam_step(*bufs, dim_ff, layers, counters, losses=losses, lr=3e-4,          # noqa: E731
                                                           betas=(0.9, 0.999), eps=1e-8, max_norm=max_norm)
                before = [t.clone() for t in bufs]
                norm1 = call(step).clone()
                check_case(name, [before], [bufs], [norm1], max_norm, skipped)
                norm2 = call(step + 1).clone()
                say("%s %s" % (name.replace(" ", "/"), digest(bufs + extra + [norm1, norm2])))


def run_ppo():
    actor, critic = state(ops.ppo_plain_floats(4), 401), state(ops.ppo_plain_floats(1), 402)
    for max_norm in MAX_NORMS:
        for gate in GATES:
            a, c = [t.clone().to(dev) for t in actor], [t.clone().to(dev) for t in critic]
            counters = torch.tensor([5, 3, 1, 2], dtype=torch.int64, device=dev)
            losses = {"no loss": None, "nan loss": torch.tensor([float("nan"), 0, 0, 0], dtype=torch.float32, device=dev)}.get(
                gate, torch.tensor([0.75, 0, 0, 0], dtype=torch.float32, device=dev))
            if gate == "inf grad":
                c[1][c[1].numel() // 3] = float("inf")
            name = "ppo max_norm=%s %s" % (max_norm, gate.replace(" ", "_"))
            before = [[t.clone() for t in a], [t.clone() for t in c]]
            call = lambda: ops.ppo_adam_step(*a, *c, counters, losses=losses, lr=(8e-4, 2e-3), betas=(0.9, 0.999), eps=(1e-8, 1e-5),      # noqa: E731
                                             max_norm=max_norm)
            norms1 = call().clone()
            check_case(name, before, [a, c], norms1.tolist(), max_norm, gate in ("nan loss", "inf grad"))
            norms2 = call().clone()
            say("%s %s" % (name.replace(" ", "/"), digest(a + c + [counters, norms1, norms2])))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    say("# main library %s; step library %s; %s" % (os.path.relpath(_lib.library_path(), REPO), os.path.relpath(_lib.tstep_library_path(), REPO),
                                                    torch.cuda.get_device_name(0)))
    for i, (dim_ff, layers) in enumerate(((32, 1), (32, 2), (32, 3), (96, 2), (2048, 2))):
        run_encoder("qnet", dim_ff, layers, state(ops.qnet_plain_floats(dim_ff, layers), 100 + i))
    for i, (dim_ff, layers) in enumerate(((32, 1), (32, 2), (32, 3), (96, 2), (4096, 2))):
        run_encoder("tpolicy", dim_ff, layers, state(ops.tpolicy_plain_floats(dim_ff, layers), 200 + i))
    run_ppo()
    say("# %d cases" % (len(LINES) - 1))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
