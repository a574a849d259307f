"""The batch passes of the three training pipelines from seeded inputs: one SHA-256 per case over every output. Two builds compute
the same bits if and only if their lists are equal:

    python3 tools/pass_digest.py [--out FILE]                              the product's libraries
    G2048_LIB=A.so G2048_TRAIN_LIB=B.so G2048_TLEARN_LIB=C.so G2048_TTRAIN_LIB=D.so python3 tools/pass_digest.py [--out FILE]
    python3 tools/pass_digest.py --host [--out FILE]                       (host, no GPU) the size queries and every refusal
    python3 tools/pass_digest.py --compare FILE FILE                       (host) the cases that differ

Entry points: g2048_qnet_forward_batch, g2048_qnet_loss_grad and their _dropout forms; g2048_tpolicy_loss_grad,
g2048_tpolicy_loss_grad_dropout, g2048_tpolicy_forward_dropout; the three *_dropout_mask; g2048_ppo_forward_train and
g2048_ppo_loss_grad with and without dropout.

Shapes: the smallest at which the shared launch code can go wrong, not the workload's. n = 1 (one tile with 15 dead rows; PPO's
path without a BatchNorm launch), 2, 15, 16, 17 (a tile edge on each side), 33 and 257 (17 row tiles: more than two groups of eight
in the tile sums); dim_ff = 32 (the minimum), 160 (one 128-chunk and a 32 tail) and 1056 (above 1024: the max(1024, dim_ff) arrays
of every workspace take the other branch); 1, 2 and 3 layers; n = 17 and 257 on every dim_ff. Dropout: none, 0.1 on all sites,
(0.3, 0, 0.2, 0.1), and (0, 0, 0, 0) THROUGH the dropout entries; call index 7 and 2^32 + 7; the mask entries also over a window of
rows that is not the whole matrix. Before it prints a digest the tool asserts that the case exercises what it names: every output
is finite, a dropout case's outputs differ in bits from the eval case's, call index 7 from 2^32 + 7, and all-zero probabilities
through a dropout entry give the eval entry's q, td, loss and gradient (probs, value, losses and gradient) bit for bit.

--host: the nine size queries over that (n, dim_ff, layers) grid and n = 0, the limit and the limit + 1, then for every entry point
the return code and the last-error string of each refusal: a null pointer, a pointer misaligned by 4 bytes, n above the limit,
dim_ff 48, n_layers 0 and 65, p of 1.0 and NaN, a null p4. Every one of these checks precedes any device call, so the addresses
passed are never read; a case that is not refused with G2048_ERR_ARG stops the tool."""
import ctypes as C
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compare(a, b):
    rows = [dict(line.rsplit(None, 1) for line in open(f) if line.strip() and not line.startswith("#")) for f in (a, b)]
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
from g2048 import _lib as L, ops  # noqa: E402

SIZES = (1, 2, 15, 16, 17, 33, 257)
# (n, dim_ff, layers): every n, every dim_ff, every depth; 17 and 257 on every dim_ff
SHAPES = ((1, 32, 2), (2, 160, 1), (15, 32, 3), (16, 160, 2), (17, 32, 1), (17, 160, 3), (17, 1056, 2), (33, 1056, 3), (257, 32, 2),
          (257, 160, 1), (257, 1056, 1))
UNEQUAL, ZEROS = (0.3, 0.0, 0.2, 0.1), (0.0, 0.0, 0.0, 0.0)
INDEX, HIGH_INDEX = 7, (1 << 32) + 7
SEED = 0x2048
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def write_out():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(LINES) + "\n")


# ------------------------------------------------------------------------------------------------------------ --host --
A, M = 0x10000, 0x10004              # a 16-byte aligned address and one misaligned by 4; never read: every case is refused first
NAN = float("nan")
ERR_ARG = -1                         # G2048_ERR_ARG (include/g2048.h)


def p4_of(*p):
    return (C.c_double * 4)(*p)


def refusals(lib, stem, name, args, cases):
    """args: {argument: value} in the entry point's order, all acceptable; cases: (label, {argument: bad value})."""
    fn, err = getattr(lib, name), getattr(lib, stem + "_last_error")
    for label, bad in cases:
        rc = fn(*[bad.get(k, v) for k, v in args.items()])
        assert rc == ERR_ARG, "%s %s: status %d, not a refusal" % (name, label, rc)
        say("refusal/%s/%s rc=%d %s" % (name, label, rc, err().decode().replace(" ", "_")))


def host():
    main, train, tlearn, ttrain, tstep = L.lib(), L.train_lib(), L.tlearn_lib(), L.ttrain_lib(), L.tstep_lib()
    say("# libraries %s" % " ".join(os.path.relpath(p(), REPO) for p in (L.library_path, L.train_library_path, L.tlearn_library_path,
                                                                         L.ttrain_library_path, L.tstep_library_path)))
    grid = sorted({(ff, layers) for _, ff, layers in SHAPES})
    for name, fn, limit in (("g2048_qnet_batch_workspace", lambda n, ff, nl: main.g2048_qnet_batch_workspace(n, ff), L.QNET_BATCH_MAX),
                            ("g2048_qnet_grad_workspace", main.g2048_qnet_grad_workspace, L.QNET_BATCH_MAX),
                            ("g2048_qnet_train_workspace", train.g2048_qnet_train_workspace, L.QNET_BATCH_MAX),
                            ("g2048_tpolicy_grad_workspace", tlearn.g2048_tpolicy_grad_workspace, L.TLEARN_BATCH_MAX),
                            ("g2048_tpolicy_train_workspace", ttrain.g2048_tpolicy_train_workspace, L.TLEARN_BATCH_MAX),
                            ("g2048_ppo_train_workspace", lambda n, ff, nl: main.g2048_ppo_train_workspace(n), L.PPO_BATCH_MAX)):
        for n in (0,) + SIZES + (limit, limit + 1):
            say("size/%s/n=%d %s" % (name, n, ",".join("%d" % fn(n, ff, nl) for ff, nl in grid)))
        say("size/%s/n=17/bad_shapes %s" % (name, ",".join("%d" % fn(17, ff, nl) for ff, nl in ((48, 2), (0, 2), (65568, 2), (32, 0), (32, 65)))))
    for name, fn in (("g2048_qnet_step_workspace", main.g2048_qnet_step_workspace), ("g2048_tpolicy_step_workspace", tstep.g2048_tpolicy_step_workspace)):
        say("size/%s %s" % (name, ",".join("%d" % fn(ff, nl) for ff, nl in grid + [(48, 2), (32, 0), (32, 65)])))
    say("size/g2048_ppo_step_workspace %d" % main.g2048_ppo_step_workspace())

    shape = [("n above the limit", {"n": L.QNET_BATCH_MAX + 1}), ("dim_ff 48", {"dim_ff": 48}), ("n_layers 0", {"n_layers": 0}),
             ("n_layers 65", {"n_layers": 65})]
    probs = [("p 1.0", {"p4": p4_of(0.1, 1.0, 0.1, 0.1)}), ("p NaN", {"p4": p4_of(0.1, 0.1, NAN, 0.1)}), ("null p4", {"p4": None})]
    ptrs = lambda first, last: [("null " + first, {first: None}), ("null " + last, {last: None}), ("misaligned " + first, {first: M})]    # noqa: E731
    fwd = dict(boards=A, plain=A, q=A, n=17, dim_ff=32, n_layers=2, workspace=A, stream=None)
    refusals(main, "g2048", "g2048_qnet_forward_batch", fwd, ptrs("boards", "workspace") + shape)
    fwd_d = dict(boards=A, plain=A, q=A, n=17, dim_ff=32, n_layers=2, p4=p4_of(0.1, 0.1, 0.1, 0.1), seed=1, call_index=7, workspace=A, stream=None)
    refusals(train, "g2048_train", "g2048_qnet_forward_batch_dropout", fwd_d, ptrs("boards", "workspace") + shape + probs)
    grad = dict(boards=A, plain=A, actions=A, targets=A, weights=A, n=17, dim_ff=32, n_layers=2, grad=A, td=A, loss=A, q=A, workspace=A, stream=None)
    more = [("misaligned actions", {"actions": M}), ("misaligned grad", {"grad": M})]
    refusals(main, "g2048", "g2048_qnet_loss_grad", grad, ptrs("boards", "loss") + more + shape)
    grad_d = dict(boards=A, plain=A, actions=A, targets=A, weights=A, n=17, dim_ff=32, n_layers=2, p4=p4_of(0.1, 0.1, 0.1, 0.1), seed=1,
                  call_index=7, grad=A, td=A, loss=A, q=A, workspace=A, stream=None)
    refusals(train, "g2048_train", "g2048_qnet_loss_grad_dropout", grad_d, ptrs("boards", "loss") + more + shape + probs)

    tshape = [("n above the limit", {"n": L.TLEARN_BATCH_MAX + 1})] + shape[1:]
    coefs = [("clip NaN", {"clip": NAN}), ("value_coef negative", {"value_coef": -1.0}), ("small workspace", {"workspace_bytes": 16})]
    tgrad = dict(boards=A, plain=A, actions=A, old=A, adv=A, ret=A, n=17, dim_ff=32, n_layers=2, clip=0.3, value_coef=0.4, ent=0.05, grad=A,
                 losses=A, probs=A, value=A, workspace=A, workspace_bytes=1 << 40, stream=None)
    refusals(tlearn, "g2048_tlearn", "g2048_tpolicy_loss_grad", tgrad, ptrs("boards", "losses") + more + tshape + coefs)
    tgrad_d = dict(boards=A, plain=A, actions=A, old=A, adv=A, ret=A, n=17, dim_ff=32, n_layers=2, p4=p4_of(0.1, 0.1, 0.1, 0.1), seed=1,
                   call_index=7, clip=0.3, value_coef=0.4, ent=0.05, grad=A, losses=A, probs=A, value=A, workspace=A, workspace_bytes=1 << 40,
                   stream=None)
    refusals(ttrain, "g2048_ttrain", "g2048_tpolicy_loss_grad_dropout", tgrad_d, ptrs("boards", "losses") + more + tshape + coefs + probs)
    tfwd_d = dict(boards=A, plain=A, n=17, dim_ff=32, n_layers=2, p4=p4_of(0.1, 0.1, 0.1, 0.1), seed=1, call_index=7, probs=A, value=A, workspace=A,
                  workspace_bytes=1 << 40, stream=None)
    refusals(ttrain, "g2048_ttrain", "g2048_tpolicy_forward_dropout", tfwd_d, ptrs("boards", "value") + tshape + coefs[2:] + probs)

    mask = dict(seed=1, call_index=7, layer=0, site=2, p=0.1, n=17, dim_ff=32, first_row=0, rows=17, keep=A, stream=None)
    mcases = [("null keep", {"keep": None}), ("dim_ff 48", {"dim_ff": 48}), ("layer 64", {"layer": 64}), ("layer -1", {"layer": -1}),
              ("site 4", {"site": 4}), ("p 1.0", {"p": 1.0}), ("p NaN", {"p": NAN}), ("rows past the end", {"first_row": 1}),
              ("first_row past the end", {"first_row": 1 << 40, "rows": 1})]
    refusals(train, "g2048_train", "g2048_qnet_dropout_mask", mask, [("n above the limit", {"n": L.QNET_BATCH_MAX + 1})] + mcases)
    refusals(ttrain, "g2048_ttrain", "g2048_tpolicy_dropout_mask", dict(mask, rows=16 * 17), [("n above the limit", {"n": L.TLEARN_BATCH_MAX + 1})] + mcases)

    pn = [("n above the limit", {"n": L.PPO_BATCH_MAX + 1})]
    pp = lambda *names: [("%s %s" % (k, label), {k: v}) for k in names for label, v in (("1.0", 1.0), ("NaN", NAN))]     # noqa: E731
    pf = dict(states=A, plain=A, running=None, n_out=4, out=A, n=17, workspace=A, stream=None)
    refusals(main, "g2048", "g2048_ppo_forward_train", pf, ptrs("states", "workspace") + pn + [("n_out 3", {"n_out": 3})])
    pf_d = dict(states=A, plain=A, running=None, n_out=4, net=0, p=0.1, seed=1, call_index=7, out=A, n=17, workspace=A, stream=None)
    refusals(main, "g2048", "g2048_ppo_forward_train_dropout", pf_d, ptrs("states", "workspace") + pn + [("net 2", {"net": 2})] + pp("p"))
    pg = dict(states=A, actions=A, old=A, adv=A, ret=A, plain_actor=A, plain_critic=A, running_actor=None, running_critic=None, clip=0.3,
              value_coef=0.4, ent=0.05, n=17, grad_actor=A, grad_critic=A, losses=A, workspace=A, stream=None)
    refusals(main, "g2048", "g2048_ppo_loss_grad", pg, ptrs("states", "losses") + pn + coefs[:2])
    pg_d = dict(list(pg.items())[:12] + [("p_actor", 0.1), ("p_critic", 0.1), ("seed", 1), ("call_index", 7)] + list(pg.items())[12:])
    refusals(main, "g2048", "g2048_ppo_loss_grad_dropout", pg_d, ptrs("states", "losses") + pn + coefs[:2] + pp("p_actor", "p_critic"))
    pm = dict(seed=1, call_index=7, net=0, site=0, p=0.1, keep=A, n=17, stream=None)
    refusals(main, "g2048", "g2048_ppo_dropout_mask", pm, [("null keep", {"keep": None}), ("net 2", {"net": 2}), ("site 2", {"site": 2})] + pn + pp("p"))
    say("# %d lines" % (len(LINES) - 1))
    write_out()


if "--host" in sys.argv:
    host()
    sys.exit(0)

# ------------------------------------------------------------------------------------------------------------ the GPU --
dev = torch.device("cuda")


def digest(tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        assert bool(torch.isfinite(t).all()), "an output is not finite"
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def bits_equal(a, b):
    return all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(a, b))


def clones(tensors):
    return [t.clone() for t in tensors]


def encoder_plain(floats, layer0, stride, layers, gen):
    """A plain parameter buffer: small normal weights, every layer's two LayerNorm-eps slots (its last two floats) 1e-5."""
    plain = torch.randn(floats, generator=gen) * 0.05
    for l in range(layers):
        plain[layer0 + (l + 1) * stride - 2:layer0 + (l + 1) * stride] = 1e-5
    return plain.to(dev)


def record(name, outs, eval_outs=None, other_index=None):
    """One line for the case; eval_outs: the eval-mode case's outputs, other_index: the same case at the other call index."""
    for label, other in (("the eval-mode case", eval_outs), ("the other call index", other_index)):
        assert other is None or not bits_equal(outs, other), "%s: the bits of %s" % (name, label)
    say("%s %s" % (name, digest(outs)))


def dropout_variants():
    """(label, p4, call index, is the 0.1 case at INDEX); the 0.1 case comes first, the other index is compared with it."""
    return (("p=0.1/c=7", (0.1,) * 4, INDEX), ("p=0.1/c=2^32+7", (0.1,) * 4, HIGH_INDEX), ("p=0.3_0_0.2_0.1/c=7", UNEQUAL, INDEX))


def run_qnet(n, ff, layers, k):
    gen = torch.Generator().manual_seed(1000 + k)
    plain = encoder_plain(ops.qnet_plain_floats(ff, layers), 139616, 66690 + 257 * ff, layers, gen)
    boards = torch.randint(0, 7, (n, 16), generator=gen, dtype=torch.uint8).to(dev)
    actions = torch.randint(0, 4, (n,), generator=gen).to(dev)
    targets, weights = torch.randn(n, generator=gen).to(dev), (torch.rand(n, generator=gen) + 0.5).to(dev)
    tag = "qnet/n=%d/ff=%d/L=%d/" % (n, ff, layers)
    q_eval = [ops.qnet_forward_batch(boards, plain, ff, layers).clone()]
    record(tag + "forward/eval", q_eval)
    g_eval = clones(ops.qnet_loss_grad(boards, plain, actions, targets, weights, ff, layers))
    assert bits_equal(g_eval[2:3], q_eval), tag + "the gradient pass's q is not the forward's"
    record(tag + "loss_grad/eval", g_eval)
    # all-zero probabilities THROUGH the dropout entries (ops sends them to the eval entries): the eval entries' bits
    q0 = torch.empty_like(q_eval[0])
    ws = torch.empty(ops.qnet_train_workspace_bytes(n, ff, layers), dtype=torch.uint8, device=dev)
    L.train_call(dev, L.train_lib().g2048_qnet_forward_batch_dropout, boards.data_ptr(), plain.data_ptr(), q0.data_ptr(), n, ff, layers, p4_of(*ZEROS),
                 SEED, INDEX, ws.data_ptr(), L.stream_ptr(dev))
    assert bits_equal([q0], q_eval), tag + "zero p4 through the forward's dropout entry"
    record(tag + "forward/p=0_through_dropout", [q0])
    loss, td, q, grad = (torch.empty_like(t) for t in g_eval)
    L.train_call(dev, L.train_lib().g2048_qnet_loss_grad_dropout, boards.data_ptr(), plain.data_ptr(), actions.data_ptr(), targets.data_ptr(),
                 weights.data_ptr(), n, ff, layers, p4_of(*ZEROS), SEED, INDEX, grad.data_ptr(), td.data_ptr(), loss.data_ptr(), q.data_ptr(),
                 ws.data_ptr(), L.stream_ptr(dev))
    assert bits_equal([loss, td, q, grad], g_eval), tag + "zero p4 through the gradient pass's dropout entry"
    record(tag + "loss_grad/p=0_through_dropout", [loss, td, q, grad])
    first = {}
    for label, p4, index in dropout_variants():
        qd = [ops.qnet_forward_batch(boards, plain, ff, layers, dropout=p4, seed=SEED, call_index=index).clone()]
        gd = clones(ops.qnet_loss_grad(boards, plain, actions, targets, weights, ff, layers, dropout=p4, seed=SEED, call_index=index))
        assert bits_equal(gd[2:3], qd), tag + label + ": the gradient pass's q is not the forward's"
        record(tag + "forward/" + label, qd, q_eval, first.get("q") if index == HIGH_INDEX else None)
        record(tag + "loss_grad/" + label, gd, g_eval, first.get("g") if index == HIGH_INDEX else None)
        first.setdefault("q", qd), first.setdefault("g", gd)


def run_tpolicy(n, ff, layers, k):
    gen = torch.Generator().manual_seed(2000 + k)
    plain = encoder_plain(ops.tpolicy_plain_floats(ff, layers), 128, 16962 + 129 * ff, layers, gen)
    boards = torch.randint(0, 12, (n, 16), generator=gen, dtype=torch.uint8).to(dev)
    actions = torch.randint(0, 4, (n,), generator=gen).to(dev)
    old = (torch.rand(n, generator=gen) * -1.5 - 0.8).to(dev)
    adv, ret = torch.randn(n, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev)
    tag = "tpolicy/n=%d/ff=%d/L=%d/" % (n, ff, layers)
    args = (boards, plain, actions, old, adv, ret, ff, layers)
    g_eval = clones(ops.tpolicy_loss_grad(*args))
    record(tag + "loss_grad/eval", g_eval)
    f0 = clones(ops.tpolicy_forward_train(boards, plain, ff, layers, None, seed=SEED, call_index=INDEX))     # zeros through the dropout entry
    assert bits_equal(f0, g_eval[1:3]), tag + "zero p4 through the forward's dropout entry"
    record(tag + "forward/p=0_through_dropout", f0)
    losses, probs, value, grad = (torch.empty_like(t) for t in g_eval)
    ws = torch.empty(ops.tpolicy_train_workspace_bytes(n, ff, layers), dtype=torch.uint8, device=dev)
    L.ttrain_call(dev, L.ttrain_lib().g2048_tpolicy_loss_grad_dropout, boards.data_ptr(), plain.data_ptr(), actions.data_ptr(), old.data_ptr(),
                  adv.data_ptr(), ret.data_ptr(), n, ff, layers, p4_of(*ZEROS), SEED, INDEX, 0.3, 0.4, 0.05, grad.data_ptr(), losses.data_ptr(),
                  probs.data_ptr(), value.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr(dev))
    assert bits_equal([losses, probs, value, grad], g_eval), tag + "zero p4 through the gradient pass's dropout entry"
    record(tag + "loss_grad/p=0_through_dropout", [losses, probs, value, grad])
    first = {}
    for label, p4, index in dropout_variants():
        fd = clones(ops.tpolicy_forward_train(boards, plain, ff, layers, p4, seed=SEED, call_index=index))
        gd = clones(ops.tpolicy_loss_grad(*args, dropout=p4, seed=SEED, call_index=index))
        assert bits_equal(gd[1:3], fd), tag + label + ": the gradient pass's probs and value are not the forward's"
        record(tag + "forward/" + label, fd, f0, first.get("f") if index == HIGH_INDEX else None)
        record(tag + "loss_grad/" + label, gd, g_eval, first.get("g") if index == HIGH_INDEX else None)
        first.setdefault("f", fd), first.setdefault("g", gd)


def run_ppo(n, k):
    gen = torch.Generator().manual_seed(3000 + k)
    actor, critic = ((torch.randn(ops.ppo_plain_floats(o), generator=gen) * 0.1).to(dev) for o in (4, 1))
    states = torch.rand(n, 16, generator=gen).to(dev)
    actions = torch.randint(0, 4, (n,), generator=gen).to(dev)
    old = (torch.rand(n, generator=gen) * -1.5 - 0.8).to(dev)
    adv, ret = torch.randn(n, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev)
    tag = "ppo/n=%d/" % n
    variants = (("eval", 0.0, INDEX), ("p=0.1/c=7", 0.1, INDEX), ("p=0.1/c=2^32+7", 0.1, HIGH_INDEX), ("p=0.3_0.2/c=7", (0.3, 0.2), INDEX))
    evals, first = {}, {}
    for label, p, index in variants:
        pa, pc = ops.ppo_pair(p, "dropout")
        outs = {}
        for net, (plain, n_out, pn) in enumerate(((actor, 4, pa), (critic, 1, pc))):
            running = torch.cat([torch.zeros(256), torch.ones(256), torch.zeros(128), torch.ones(128)]).to(dev)
            out = ops.ppo_forward_train(states, plain, n_out, running=running, dropout=pn, seed=SEED, call_index=index, net=net).clone()
            outs["forward_%s" % ("actor", "critic")[net]] = [out, running]
        ra, rc = (torch.cat([torch.zeros(256), torch.ones(256), torch.zeros(128), torch.ones(128)]).to(dev) for _ in range(2))
        outs["loss_grad"] = clones(ops.ppo_loss_grad(states, actions, old, adv, ret, actor, critic, ra, rc, dropout=p, seed=SEED,
                                                     call_index=index)) + [ra, rc]
        for what, o in outs.items():
            record(tag + what + "/" + label, o, evals.get(what), first.get(what) if index == HIGH_INDEX else None)
            if label == "eval":
                evals[what] = o
            elif label == "p=0.1/c=7":
                first[what] = o


def run_masks():
    for kind, fn, shape in (("qnet", ops.qnet_dropout_mask, lambda s, n, ff: (8 * n, n) if s == 0 else (n, ff if s == 2 else 128)),
                            ("tpolicy", ops.tpolicy_dropout_mask, lambda s, n, ff: (64 * n, 16) if s == 0 else (16 * n, ff if s == 2 else 64))):
        for n, ff in ((1, 32), (17, 160), (257, 1056)):
            for site in range(4):
                height = shape(site, n, ff)[0]
                whole = {}
                for index in (INDEX, HIGH_INDEX):
                    whole[index] = fn(n, 2, site, 0.3, dim_ff=ff, seed=SEED, call_index=index)
                    assert tuple(whole[index].shape) == shape(site, n, ff)
                    record("mask/%s/n=%d/ff=%d/site=%d/c=%d/whole" % (kind, n, ff, site, index), [whole[index]],
                           other_index=[whole[INDEX]] if index == HIGH_INDEX else None)
                first, rows = height // 3, max(1, height // 2)
                window = fn(n, 2, site, 0.3, dim_ff=ff, seed=SEED, call_index=INDEX, first_row=first, rows=rows)
                assert bits_equal([window], [whole[INDEX][first:first + rows]]), "a window of rows is not the whole matrix's rows"
                record("mask/%s/n=%d/ff=%d/site=%d/c=%d/rows=%d+%d" % (kind, n, ff, site, INDEX, first, rows), [window])
    for n in (1, 17, 257):
        for net in (0, 1):
            for site in (0, 1):
                both = [ops.ppo_dropout_mask(n, net, site, 0.3, seed=SEED, call_index=index) for index in (INDEX, HIGH_INDEX)]
                record("mask/ppo/n=%d/net=%d/site=%d/c=%d" % (n, net, site, INDEX), both[:1])
                record("mask/ppo/n=%d/net=%d/site=%d/c=%d" % (n, net, site, HIGH_INDEX), both[1:], other_index=both[:1])


def main():
    say("# libraries %s; %s" % (" ".join(os.path.relpath(p(), REPO) for p in (L.library_path, L.train_library_path, L.tlearn_library_path,
                                                                              L.ttrain_library_path)), torch.cuda.get_device_name(0)))
    for k, (n, ff, layers) in enumerate(SHAPES):
        run_qnet(n, ff, layers, k)
        run_tpolicy(n, ff, layers, k)
    for k, n in enumerate(SIZES):
        run_ppo(n, k)
    run_masks()
    say("# %d cases" % (len(LINES) - 1))
    write_out()


if __name__ == "__main__":
    main()
