"""g2048_tpolicy_adam_step on the MI355X: the NaN gate on the loss, gradient clipping and Adam over the transformer policy's plain
buffer in three launches, and DeviceTransformerPolicy.adam_step / update / optimizer_state_dict / load_optimizer_state_dict around it.

The kernel is checked against the yardstick tpolicy_step_ref.adam_step_reference (itself clip_grad_norm_ + torch.optim.Adam to 1e-12
per tensor: tests/test_tpolicy_step_host.py). Tolerance, the convention of tests/test_gpu_ppo_step.py: per buffer max|device - y64| /
max|y64| <= 8 x the same measure of the float32 yardstick, both yardsticks fed the device's own pre-step state; the float32 deviation
must be > 0. The norm is held to 1e-6 of the float64 norm of the device's gradient, a clipped gradient to 4 float32 ulps an element
of grad . c with c formed in float64 from the device's own norm, an unclipped one to its bits.

Shapes (dim_ff, layers): (32, 1) 160,999 floats, a tail group of 3 floats and one eps pair; (96, 2) 198,601 floats, a tail of 1 float
and the eps pairs in both halves of a group; (2048, 2) the reference's; (4096, 2) 1,230,601 floats, where a norm block makes two passes.
Every buffer the entry point is given lies between the bands of tests/guard.py, in every test.

Measured on an MI355X (docs/LOG.md R30.1): the four-step case 1.00 x the float32 yardstick's deviation on weights and both moments at
all four shapes; with moments as after a few steps at most 1.39 x; clipped gradients within 1.25 float32 ulps; 22 tests in 8 s."""
import contextlib
import copy
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

import guard
import tpolicy_grad_ref as R
import tpolicy_step_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
KW = dict(lr=T.LR, eps=T.EPS, max_norm=T.MAX_NORM, betas=T.BETAS)
NAMES = ("plain", "grad", "exp_avg", "exp_avg_sq")
SMALL = ((32, 1), (96, 2))
SMALL_IDS = ["ff32-L1-tail3", "ff96-L2-tail1"]


def bits(t):
    return guard.bits(t)


@contextlib.contextmanager
def no_sync():
    """Inside, a torch operation that synchronises with the host raises."""
    torch.cuda.synchronize()
    with warnings.catch_warnings():                      # torch says that the mode is a prototype
        warnings.simplefilter("ignore")
        torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


class Guarded:
    """The four buffers, the norm, the counters and the workspace (of exactly the size the query gives) as regions of a guard.Set:
    bands round each of them. The weights start as the case's, the moments and counters as zeros, the norm as 7."""

    def __init__(self, dim_ff, layers, s=None):
        from g2048 import ops
        self.shape = (dim_ff, layers)
        self.set = s if s is not None else guard.Set(0xFF, 0x3C, DEV)          # bands of NaN round the float buffers
        plain, _ = T.step_case(dim_ff, layers)
        zeros = torch.zeros_like(plain)
        self.buffers = [self.set.inp(name, data, align=16) for name, data in zip(NAMES, (plain, zeros, zeros, zeros))]
        self.norm = self.set.inp("norm", torch.full((1,), 7.0), align=4)
        self.counters = self.set.inp("counters", torch.zeros(3, dtype=torch.int64), align=8)
        self.nb = ops.tpolicy_step_workspace_bytes(dim_ff, layers)
        self.workspace = self.set.out("workspace", self.nb, (), torch.uint8, align=16)
        self.eps_at = T.eps_slots(dim_ff, layers)

    def set_grad(self, grad):
        self.buffers[1].copy_(grad)

    def set_moments(self, grads):
        """Moments as a few steps would leave them: exp_avg = 0.1 x a gradient, exp_avg_sq = the square of another."""
        self.buffers[2].copy_(grads[1] * 0.1)
        self.buffers[3].copy_(grads[2] * grads[2])

    def pre(self):
        return [t.cpu().clone() for t in self.buffers]

    def all_bits(self):
        return [bits(t).clone() for t in self.buffers]

    def step(self, losses=None, **kw):
        from g2048 import ops
        if isinstance(losses, (list, tuple)):
            losses = torch.tensor(losses, dtype=torch.float32, device=DEV)
        out = ops.tpolicy_adam_step(*self.buffers, *self.shape, self.counters, losses=losses, norm=self.norm, workspace=self.workspace,
                                    **dict(KW, **kw))
        assert out is self.norm
        torch.cuda.synchronize()
        self.set.check()
        return out


def check_norm(norm, grad_pre, what):
    norm64 = float(np.linalg.norm(grad_pre.numpy().astype(np.float64)))
    assert abs(float(norm) - norm64) <= 1e-6 * norm64, (what, float(norm), norm64)
    return norm64


def check_buffers(pre, post, eps_at, step, what, want=None, **kw):
    """The post-step buffers against both yardsticks run from the pre-step buffers (want: another float64 truth in the yardstick's
    place): the bound on weights and moments. Returns the three multiples of the float32 yardstick's deviation."""
    y64, y32 = T.yardsticks(pre, eps_at, step, **kw)
    if want is not None:
        y64 = want
    row = []
    for i in (0, 2, 3):
        e_dev, e_f32 = T.deviation(post[i].numpy(), y64[i]), T.deviation(y32[i], y64[i])
        row.append(e_dev / e_f32 if e_f32 > 0 else np.inf)
        print("%s: %s %.3g of the largest entry from the float64 yardstick = %.2f x the float32 yardstick's %.3g (bound %.0f x)"
              % (what, NAMES[i], e_dev, row[-1], e_f32, T.F32_FACTOR))
        assert e_f32 > 0 and e_dev <= T.F32_FACTOR * e_f32, (what, NAMES[i])
    return row


def check_clipped_gradient(norm, g_pre, g_post, clipped, what):
    coef = T.clip_coefficient(float(norm))
    assert (coef < 1.0) == clipped, (what, coef)
    g_pre, g_post = g_pre.numpy(), g_post.numpy()
    if coef == 1.0:
        assert np.array_equal(g_post.view(np.int32), g_pre.view(np.int32)), "%s: an unclipped gradient changed" % what
        return
    want = g_pre.astype(np.float64) * coef
    ulps = np.abs(g_post.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print("%s: clipped gradient within %.2f float32 ulps of grad . c (c = %.9g)" % (what, ulps.max(), coef))
    assert ulps.max() <= 4.0, what


def check_slots_kept(pre, post, eps_at, what):
    for name, a, b in zip(NAMES, pre, post):
        assert torch.equal(bits(a[eps_at]), bits(b[eps_at])), "%s: a LayerNorm-eps slot of %s changed" % (what, name)


# ------------------------------------------------------------------------------------------------------ the entry point --
@pytest.mark.parametrize("dim_ff, layers", T.SHAPES, ids=["ff32-L1-tail3", "ff96-L2-tail1", "reference-shape", "two-passes-a-block"])
def test_four_steps_against_the_yardstick(dim_ff, layers):
    """The gradient's norm runs 2, 1, 0.5, 0.5 x max_norm: clipped, clipped at the edge, unclipped twice. Every step: the norm within
    1e-6 of the float64 norm, weights and moments within 8 x the float32 yardstick's deviation, the gradient left clipped (4 ulps) or
    bit-equal, the eps slots' bits kept, the last float (the short tail group) moved by about lr in step 1, the bands intact.
    Measured on an MI355X: weights, exp_avg and exp_avg_sq 1.00 x at every shape and step (weights 2.9e-8 .. 3.2e-8 of max|w|); the
    clipped gradients within 1.25 ulps at c = 0.4999995 and 0.94 at c = 0.999998."""
    _, grads = T.step_case(dim_ff, layers)
    c = Guarded(dim_ff, layers)
    ratios = []
    for s in range(4):
        c.set_grad(grads[s])
        pre = c.pre()
        c.step()
        post = c.pre()
        what = "dim_ff %d, %d layers, step %d" % (dim_ff, layers, s + 1)
        norm64 = check_norm(c.norm[0], pre[1], what)
        assert norm64 == pytest.approx(T.FACTORS[s] * T.MAX_NORM, rel=1e-6)
        ratios.append(check_buffers(pre, post, c.eps_at, s + 1, what))
        check_clipped_gradient(c.norm[0], pre[1], post[1], T.FACTORS[s] >= 1.0, what)
        check_slots_kept(pre, post, c.eps_at, what)
        if s == 0:          # critic.bias, in the short tail group: a first Adam step of about lr
            moved = abs(float(post[0][-1].double() - pre[0][-1].double()))
            assert 0.5 * T.LR < moved < 1.5 * T.LR, moved
    assert c.counters.tolist() == [4, 0, 0]
    print("dim_ff %d, %d layers: worst multiple of the float32 yardstick's deviation %.2f" % (dim_ff, layers, max(max(r) for r in ratios)))


@pytest.mark.parametrize("dim_ff, layers", SMALL, ids=SMALL_IDS)
def test_eps_slots_keep_their_bits_and_their_neighbours_move(dim_ff, layers):
    """Distinct non-zero values in the eps slots of plain, exp_avg and exp_avg_sq, 0 in grad's: after an applied (clipping) step all
    2 L slots of all four buffers keep their bits, and the floats on both sides of every pair changed in all four."""
    _, grads = T.step_case(dim_ff, layers)
    c = Guarded(dim_ff, layers)
    c.set_grad(grads[0])
    c.set_moments(grads)
    at = torch.from_numpy(c.eps_at)
    for k, i in enumerate((0, 2, 3)):
        c.buffers[i][at.to(DEV)] = (torch.arange(len(at), dtype=torch.float32) * 0.37 + 1.5 + k).to(DEV)
    pre = c.pre()
    c.step()
    post = c.pre()
    assert c.counters.tolist() == [1, 0, 0]
    check_slots_kept(pre, post, c.eps_at, "applied step")
    assert not post[1][at].any()
    pairs = c.eps_at.reshape(-1, 2)
    beside = torch.from_numpy(np.concatenate([pairs[:, 0] - 1, pairs[:, 1] + 1]))
    for name, a, b in zip(NAMES, pre, post):
        assert bool((bits(a[beside]) != bits(b[beside])).all()), "%s: a float next to an eps pair did not change" % name
    check_buffers(pre, post, c.eps_at, 1, "eps slots set, dim_ff %d" % dim_ff)


def gate_call(dim_ff, layers, losses, poison=None):
    """One call from the same start (moments as after a few steps, counters {5, 1, 2}): (pre buffers, post bits, norm bits,
    counters)."""
    _, grads = T.step_case(dim_ff, layers)
    c = Guarded(dim_ff, layers)
    c.set_grad(grads[0])
    c.set_moments(grads)
    c.counters.copy_(torch.tensor([5, 1, 2]))
    if poison is not None:
        c.buffers[1][-1] = poison
    pre = c.pre()
    c.step(losses=losses)
    return pre, c.pre(), bits(c.norm).clone(), c.counters.tolist()


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("dim_ff, layers", SMALL, ids=SMALL_IDS)
def test_the_skip_rules(dim_ff, layers):
    """losses=None is applied at step 6; a NaN loss[0] over a finite gradient changes nothing and counts in counters[1], the norm
    still written; +inf and -inf are applied (isnan only, the reference's rule), as is a NaN in loss[1..3]: the ungated call's bits.
    A NaN, and an inf, in the LAST float of grad (the short tail group) changes nothing and counts in counters[2]; the norm written
    is not finite. A NaN loss AND a gradient that is not finite count as a NaN loss."""
    pre, base, norm, counters = gate_call(dim_ff, layers, None)
    assert counters == [6, 1, 2]
    check_buffers(pre, base, T.eps_slots(dim_ff, layers), 6, "losses=None at step 6")
    seven = bits(torch.tensor([7.0]))

    _, post, norm_nan, counters = gate_call(dim_ff, layers, [NAN, 1.0, 1.0, 1.0])
    assert same(post, pre), "a NaN loss changed a buffer"
    assert counters == [5, 2, 2] and torch.equal(norm_nan, norm)

    for what, losses in (("+inf loss", [INF, 1.0, 1.0, 1.0]), ("-inf loss", [-INF, 1.0, 1.0, 1.0]), ("NaN in loss[1..3]", [0.25, NAN, NAN, NAN]),
                         ("a finite loss", [0.25, 0.1, 0.3, 1.2])):
        _, post, norm_k, counters = gate_call(dim_ff, layers, losses)
        assert same(post, base), "%s: not the ungated call's bits" % what
        assert counters == [6, 1, 2] and torch.equal(norm_k, norm), what

    for poison in (NAN, INF):
        pre_p, post, norm_p, counters = gate_call(dim_ff, layers, [0.25, 0.0, 0.0, 0.0], poison=poison)
        assert same(post, pre_p), "a buffer changed although the norm is not finite"
        assert counters == [5, 1, 3], poison
        assert not torch.equal(norm_p, seven) and not np.isfinite(norm_p.view(torch.float32).item()), "norm_out is written on a skipped call"
    _, post, _, counters = gate_call(dim_ff, layers, [NAN, 0.0, 0.0, 0.0], poison=NAN)
    assert counters == [5, 2, 2]


@pytest.mark.parametrize("dim_ff, layers", SMALL, ids=SMALL_IDS)
def test_the_step_number_is_the_devices(dim_ff, layers):
    """apply, skip (NaN loss), apply: the third call is Adam step 2 and meets the bound against the yardstick at step 2.
    tests/test_tpolicy_step_host.py asserts that the yardstick at step 3 is more than twice the bound away, so counting the skipped
    call cannot pass. The whole sequence also meets the bound against the yardstick run with step numbers 1 and 2 from the start."""
    _, grads = T.step_case(dim_ff, layers)
    c = Guarded(dim_ff, layers)
    c.set_grad(grads[0])
    c.step(losses=[0.5, 0, 0, 0])
    c.set_grad(grads[1])
    held = c.all_bits()
    c.step(losses=[NAN, 0, 0, 0])
    assert all(torch.equal(a, b) for a, b in zip(held, c.all_bits())) and c.counters.tolist() == [1, 1, 0]
    pre = c.pre()
    c.step(losses=[0.5, 0, 0, 0])
    post = c.pre()
    assert c.counters.tolist() == [2, 1, 0]
    check_buffers(pre, post, c.eps_at, 2, "apply, skip, apply against step 2")
    want, f32 = T.run_reference(dim_ff, layers, (0, 1), (1, 2)), T.run_reference(dim_ff, layers, (0, 1), (1, 2), dtype=torch.float32)
    for i in (0, 2, 3):
        e_dev, e_f32 = T.deviation(post[i].numpy(), want[i]), T.deviation(f32[i], want[i])
        print("the sequence, %s: %.2f x the float32 yardstick's %.3g" % (NAMES[i], e_dev / e_f32, e_f32))
        assert e_f32 > 0 and e_dev <= T.F32_FACTOR * e_f32


@pytest.mark.parametrize("dim_ff, layers", SMALL, ids=SMALL_IDS)
def test_guard_bands_round_everything_the_entry_point_writes(dim_ff, layers):
    """The two-run protocol of tests/guard.py on an applied and on a skipped call: the four buffers, the norm, the counters and the
    workspace (sized by the query exactly) between bands that must stay intact, and both runs (bands and workspace prefill of 0x00 /
    0x3C, then 0xFF / 0xC3) bit-equal: nothing outside what the call was given reaches a result, and no workspace byte is read
    before the call wrote it."""
    _, grads = T.step_case(dim_ff, layers)
    for what, losses, counters in (("applied", [0.5, 0, 0, 0], [4, 0, 0]), ("skipped", [NAN, 0, 0, 0], [3, 1, 0])):
        def call(s):
            c = Guarded(dim_ff, layers, s)
            c.set_grad(grads[0])
            c.set_moments(grads)
            c.counters.copy_(torch.tensor([3, 0, 0]))
            c.step(losses=losses)
            return dict(zip(NAMES, c.buffers), norm=c.norm, counters=c.counters)

        out = guard.twice(DEV, call)
        assert out["counters"].tolist() == counters, what
        check_norm(out["norm"][0], grads[0], what)


def test_two_runs_give_the_same_bits_and_no_clipping_keeps_the_gradient():
    """Two runs of the four steps from the same state: the same bits in every buffer and in every norm. max_norm=None: the gradient
    keeps its bits however large its norm, and the step meets the bound against the yardstick without clipping."""
    dim_ff, layers = 96, 2
    _, grads = T.step_case(dim_ff, layers)
    runs = []
    for _ in range(2):
        c, norms = Guarded(dim_ff, layers), []
        for s in range(4):
            c.set_grad(grads[s])
            c.step()
            norms.append(bits(c.norm).clone())
        runs.append(c.all_bits() + norms)
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two runs from the same state differ"
    c = Guarded(dim_ff, layers)
    c.set_grad(grads[0] * 64.0)
    pre = c.pre()
    c.step(max_norm=None)
    post = c.pre()
    assert torch.equal(bits(pre[1]), bits(post[1])), "max_norm=None changed the gradient"
    check_norm(c.norm[0], pre[1], "no clipping")
    check_buffers(pre, post, c.eps_at, 1, "max_norm=None", max_norm=None)


def test_the_clip_takes_the_reciprocal_first():
    """c = fminf(1, (1 / (norm + 1e-6f)) max_norm), the reciprocal first, as torch evaluates max_norm / tensor. At PPOAgent's 0.5 the
    direct quotient gives the same bits; at max_norm 0.3 and these gradients the two forms differ (asserted, from the device's own
    norm), and the gradient left behind is grad . c of the reciprocal-first form bit for bit: one float32 product an element."""
    dim_ff, layers = 96, 2
    _, grads = T.step_case(dim_ff, layers)
    for scale in T.CLIP_FORM_SCALES:
        c = Guarded(dim_ff, layers)
        c.set_grad(grads[1] * np.float32(scale))
        pre = c.pre()
        c.step(max_norm=T.CLIP_FORM_MAX_NORM)
        post = c.pre()
        norm = np.float32(float(c.norm[0]))
        check_norm(norm, pre[1], "scale %g" % scale)
        first, direct = T.clip_forms(norm, T.CLIP_FORM_MAX_NORM)
        assert first != direct, "the case does not tell the two forms apart"
        want = pre[1].numpy() * first
        want[c.eps_at] = pre[1].numpy()[c.eps_at]
        assert np.array_equal(post[1].numpy().view(np.int32), want.view(np.int32)), "scale %g: grad is not grad . c of the reciprocal-first form" % scale
        check_buffers(pre, post, c.eps_at, 1, "max_norm 0.3, scale %g" % scale, max_norm=T.CLIP_FORM_MAX_NORM)


# ----------------------------------------------------------------------------------------------------------- the wrapper --
N_WRAP, FF_WRAP, L_WRAP = 17, 96, 2


def device_net(model32, precision="f32"):
    from g2048 import DeviceTransformerPolicy
    return DeviceTransformerPolicy(copy.deepcopy(model32).to(DEV).eval(), precision)


def to_dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in arrays)


def update_inputs():
    """(boards, actions, old_log_probs, rewards, next_boards, dones) of the wrapper's case: tpolicy_grad_ref's (17, 96, 2), the
    boards rolled by one as their successors."""
    c = R.case(N_WRAP, FF_WRAP, L_WRAP)
    i = np.arange(c.n)
    rewards = (c.ret * 0.5 + (i % 3)).astype(np.float32)
    dones = (i % 5 == 0).astype(np.float32)
    boards, actions, old, rewards, nxt, dones = to_dev(c.boards, c.actions, c.old, rewards, np.roll(c.boards, 1, axis=0), dones)
    return c, (boards, actions, old, rewards, nxt, dones)


def net_state(net):
    return [net.plain, net.grad, net.exp_avg, net.exp_avg_sq, net.packed, net.opt_counters]


def module_equals_plain(net):
    o = 0
    for t in net.parsed.plain_tensors():
        if isinstance(t, torch.Tensor):
            if not torch.equal(bits(net.plain[o:o + t.numel()]), bits(t.reshape(-1))):
                return False
            o += t.numel()
        else:
            o += 1
    return True


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("attach", [True, False], ids=["attached", "loose"])
def test_update_is_its_parts_and_reads_nothing_back(precision, attach):
    """update(epochs=3) leaves the bits of advantages(), then loss_and_grad and adam_step three times, called one by one on a twin
    network: plain, grad, the moments, the packed blob, the counters, and the rows of losses and norms. After one warm-up call it
    raises nothing with torch's synchronisation check set to raise. Afterwards packed equals a fresh pack of plain at the network's
    precision and the module's parameters equal plain bit for bit, attached or not."""
    from g2048 import ops
    c, inputs = update_inputs()
    boards, actions, old, rewards, nxt, dones = inputs
    net, twin = device_net(c.model32, precision), device_net(c.model32, precision)
    if attach:
        net.attach_params()
        twin.attach_params()
    ret, adv = twin.advantages(boards, nxt, rewards, dones)
    rows = []
    for _ in range(3):
        losses, _, _ = twin.loss_and_grad(boards, actions, old, adv, ret)
        norm = twin.adam_step(losses, **KW)
        assert norm.dtype == torch.float32 and norm.is_cuda and norm.numel() == 1
        rows.append((bits(losses).clone(), bits(norm).clone()))
    want = [t.clone() for t in net_state(twin)]

    start = [t.clone() for t in net_state(net)]
    net.update(*inputs, epochs=3, **KW)                  # the warm-up call: buffers are allocated
    for t, s in zip(net_state(net), start):
        t.copy_(s)
    with no_sync():
        losses, norms = net.update(*inputs, epochs=3, **KW)
    torch.cuda.synchronize()
    assert losses.shape == (3, 4) and norms.shape == (3,) and losses.is_cuda and norms.is_cuda
    for name, a, b in zip(NAMES + ("packed", "opt_counters"), net_state(net), want):
        assert torch.equal(bits(a), bits(b)), "update() and the manual sequence leave other bits in %s" % name
    for e, (lb, nb) in enumerate(rows):
        assert torch.equal(bits(losses[e]), lb) and torch.equal(bits(norms[e]).reshape(-1), nb.reshape(-1)), "epoch %d" % e
    assert net.opt_counters.tolist() == [3, 0, 0] and np.isfinite(losses.cpu().numpy()).all()
    assert not torch.equal(net.plain, start[0])
    assert torch.equal(net.packed, ops.tpolicy_pack(net.plain, net.dim_ff, net.n_layers, precision)), "packed is not a pack of plain"
    assert net.params_attached == attach and module_equals_plain(net) and module_equals_plain(twin)
    with pytest.raises(TypeError, match="unexpected arguments"):
        net.update(*inputs, epochs=1, weight_decay=0.1)
    with pytest.raises(ValueError, match="at least one epoch"):
        net.update(*inputs, epochs=0)


def test_a_captured_forward_replays_with_the_new_weights():
    """A forward captured in a single-stream graph BEFORE adam_step: after the step the replay gives the output of a fresh forward
    on the new weights, which differs from the old: adam_step packs in place."""
    c, inputs = update_inputs()
    boards, actions, old, rewards, nxt, dones = inputs
    net = device_net(c.model32)
    net.attach_params()
    ret, adv = net.advantages(boards, nxt, rewards, dones)
    net(boards)                                          # the output buffers exist before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        net(boards)
        with torch.cuda.graph(graph, stream=side):
            probs, value = net(boards)
        graph.replay()
        side.synchronize()
        old_probs = probs.clone()
        losses, _, _ = net.loss_and_grad(boards, actions, old, adv, ret)
        net.adam_step(losses, **dict(KW, lr=1e-2))
        graph.replay()
        side.synchronize()
        replayed = (probs.clone(), value.clone())
    torch.cuda.current_stream(DEV).wait_stream(side)
    fresh = device_net(net.model)(boards)
    torch.cuda.synchronize()
    assert torch.equal(bits(replayed[0]), bits(fresh[0])) and torch.equal(bits(replayed[1]), bits(fresh[1]))
    assert not torch.equal(replayed[0], old_probs), "the step changed nothing the forward can see"
    assert net.opt_counters.tolist() == [1, 0, 0]


# -------------------------------------------------------------------------------------------------------- the state dict --
class FcFirstSpelling(nn.Module):
    """The reference's structure with the fc layers and the heads registered BEFORE the encoder: model.parameters() is not the plain
    order."""

    def __init__(self, dim_ff, num_layers):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(1024, 128), nn.Linear(128, 64)
        self.critic, self.actor = nn.Linear(64, 1), nn.Linear(64, 4)
        layer = nn.TransformerEncoderLayer(d_model=64, nhead=4, dim_feedforward=dim_ff, batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=num_layers, enable_nested_tensor=False)
        self.embedding = nn.Linear(1, 64)

    def forward(self, x):
        n = x.size(0)
        x = self.transformer_encoder(self.embedding(x.view(n, 16, 1))).reshape(n, -1)
        x = torch.relu(self.fc2(torch.relu(self.fc1(x))))
        return torch.softmax(self.actor(x), dim=-1), self.critic(x)


def spelled(kind):
    """The (96, 2) case's float32 module, as the reference spells it or with the fc layers first (the same weights by name)."""
    stock = T.module_of(FF_WRAP, L_WRAP)
    if kind == "reference":
        return copy.deepcopy(stock)
    model = FcFirstSpelling(FF_WRAP, L_WRAP)
    model.load_state_dict(stock.state_dict())
    return model.eval()


def offsets_by_identity(parsed, module):
    """[(parameter, offset into the plain layout)] in module.parameters() order."""
    at, o = {}, 0
    for t in parsed.plain_tensors():
        if isinstance(t, torch.Tensor):
            at[id(t)] = o
            o += t.numel()
        else:
            o += 1
    return [(p, at[id(p)]) for p in module.parameters()]


def scatter(pairs, tensors, base):
    """The per-parameter tensors at their plain offsets over a copy of `base` (float64 NumPy)."""
    out = torch.as_tensor(base).double().numpy().copy()
    for (p, o), t in zip(pairs, tensors):
        out[o:o + p.numel()] = t.detach().reshape(-1).double().numpy()
    return out


def set_grads(pairs, flat, dtype):
    for p, o in pairs:
        p.grad = flat[o:o + p.numel()].to(dtype).view(p.shape).clone()


def buffers_of(net):
    return [t.cpu().clone() for t in (net.plain, net.grad, net.exp_avg, net.exp_avg_sq)]


@pytest.mark.parametrize("kind", ["reference", "fc-first"])
def test_checkpoint_interop_with_torch_optim_adam(kind):
    """Empty before the first step. After two device steps optimizer_state_dict() loads into a fresh torch.optim.Adam over a float64
    deep copy of the module; its third step (stock clip_grad_norm_ + step) and the device's third step from the same gradient agree
    within the four-step test's bound. The other way: a stock float32 optimizer's state after two stock steps, loaded into a fresh
    network, lands at each parameter's plain offset and continues on the device as step 3. With the fc layers registered before
    the encoder, model.parameters() order is not the plain order and both directions still hold."""
    _, grads = T.step_case(FF_WRAP, L_WRAP)
    eps_at = T.eps_slots(FF_WRAP, L_WRAP)
    net = device_net(spelled(kind))
    net.attach_params()
    sd = net.optimizer_state_dict()
    assert sd["state"] == {} and sd["param_groups"][0]["params"] == list(range(34)) and sd["param_groups"][0]["lr"] == 3e-4
    for s in (0, 1):
        net.grad.copy_(grads[s])
        net.adam_step(None, **dict(KW, lr=2e-4))
    sd = net.optimizer_state_dict()
    assert sorted(sd["state"]) == list(range(34)) and sd["state"][0]["step"] == 2 and net.opt_counters.tolist() == [2, 0, 0]
    assert sd["param_groups"][0]["lr"] == 2e-4 and sd["param_groups"][0]["eps"] == T.EPS
    m64 = copy.deepcopy(net.model).cpu().double()
    from g2048 import tpolicy
    pairs64 = offsets_by_identity(tpolicy.parse(m64), m64)
    if kind == "fc-first":
        assert [o for _, o in pairs64] != sorted(o for _, o in pairs64), "the spelling's parameter order is the plain order"
    assert [tuple(sd["state"][i]["exp_avg"].shape) for i in range(34)] == [tuple(p.shape) for p, _ in pairs64]
    opt = torch.optim.Adam(m64.parameters(), lr=123.0)
    opt.load_state_dict(sd)
    net.grad.copy_(grads[2])
    pre = buffers_of(net)
    net.adam_step(None, **dict(KW, lr=2e-4))
    post = buffers_of(net)
    set_grads(pairs64, grads[2], torch.float64)
    torch.nn.utils.clip_grad_norm_(list(m64.parameters()), T.MAX_NORM)
    opt.step()
    params = [p for p, _ in pairs64]
    assert all(int(opt.state[p]["step"]) == 3 for p in params) and opt.param_groups[0]["lr"] == 2e-4
    want = (scatter(pairs64, params, pre[0]), None, scatter(pairs64, [opt.state[p]["exp_avg"] for p in params], pre[2]),
            scatter(pairs64, [opt.state[p]["exp_avg_sq"] for p in params], pre[3]))
    check_buffers(pre, post, eps_at, 3, "%s, third step against the stock float64 optimizer" % kind, want=want, lr=2e-4)

    # the other way
    model = spelled(kind)
    pairs = offsets_by_identity(tpolicy.parse(model), model)
    stock = torch.optim.Adam(model.parameters(), lr=T.LR, eps=T.EPS)
    for s in (0, 1):
        set_grads(pairs, grads[s], torch.float32)
        torch.nn.utils.clip_grad_norm_(list(model.parameters()), T.MAX_NORM)
        stock.step()
    fresh = device_net(model)
    fresh.attach_params()
    fresh.load_optimizer_state_dict(stock.state_dict())
    assert fresh.opt_counters.tolist() == [2, 0, 0]
    zeros = np.zeros(fresh.plain.numel())
    assert np.array_equal(fresh.exp_avg.cpu().numpy(), scatter(pairs, [stock.state[p]["exp_avg"] for p, _ in pairs], zeros))
    assert np.array_equal(fresh.exp_avg_sq.cpu().numpy(), scatter(pairs, [stock.state[p]["exp_avg_sq"] for p, _ in pairs], zeros))
    fresh.grad.copy_(grads[2])
    pre = buffers_of(fresh)
    fresh.adam_step(None, **KW)
    check_buffers(pre, buffers_of(fresh), eps_at, 3, "%s, continued from a stock optimizer's state" % kind)
    assert fresh.opt_counters.tolist() == [3, 0, 0]
    # a fresh optimizer's (empty) state resets; the refusals
    fresh.load_optimizer_state_dict(torch.optim.Adam(model.parameters()).state_dict())
    assert fresh.opt_counters.tolist() == [0, 0, 0] and not fresh.exp_avg.any() and not fresh.exp_avg_sq.any()
    for bad in (dict(amsgrad=True), dict(maximize=True), dict(weight_decay=0.01)):
        with pytest.raises(ValueError, match="amsgrad, maximize and weight_decay"):
            fresh.load_optimizer_state_dict(torch.optim.Adam(model.parameters(), **bad).state_dict())
    with pytest.raises(ValueError, match="one parameter group of 34"):
        fresh.load_optimizer_state_dict(torch.optim.Adam(list(model.parameters())[:5]).state_dict())
    other = torch.optim.Adam(list(reversed(list(model.parameters()))))
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    other.step()
    with pytest.raises(ValueError, match="shape"):
        fresh.load_optimizer_state_dict(other.state_dict())


def test_example_updates_with_the_device_optimizer():
    """examples/tpolicy_update.py --optimizer device (the default): every update is one net.update() call; the losses are finite and
    every epoch's Adam step is applied."""
    import os
    import re
    import subprocess
    import sys
    from conftest import REPO
    script = os.path.join(REPO, "examples", "tpolicy_update.py")
    out = subprocess.run([sys.executable, script, "--envs", "64", "--updates", "2", "--epochs", "2", "--dim-ff", "96", "--optimizer", "device"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = re.findall(r"update \d: 64 boards, last epoch's loss (\S+) = actor (\S+) \+ 0.4 x value (\S+) - 0.05 x entropy (\S+);", out.stdout)
    assert len(lines) == 2 and all(np.isfinite(float(v)) for row in lines for v in row), out.stdout[-2000:]
    counts = re.search(r"device optimizer: (\d+) Adam steps applied, (\d+) epochs skipped for a NaN loss, (\d+) for", out.stdout)
    assert counts and [int(v) for v in counts.groups()] == [4, 0, 0], out.stdout[-2000:]
