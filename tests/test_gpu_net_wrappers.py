"""The contract the three device networks (DevicePolicy with a critic, DeviceTransformerPolicy, DeviceQNetwork) share, on the
MI355X: the outputs are buffers the network owns, one set per (N, stream); refresh() flattens and packs in place; and a call is
nothing but the direct ops.*_forward launch on the module's packed weights. N = 1, 17 and 33 straddle the transformer kernel's
16-board block and the Q-network's 32-board wavefront. Every comparison is exact."""
import pytest
import torch

import test_qnet_host
import test_tpolicy_host
from test_policy_host import RefLayout, perturb_bn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 17, 33)
KEYS = dict(seed=77, step_index=5, id_base=1 << 33)


def as_tuple(out):
    return out if isinstance(out, tuple) else (out,)


def make_policy(precision):
    """(network, direct(boards) from freshly folded and packed blobs, its plain buffers, its packed blobs)"""
    from g2048 import DevicePolicy, ops, policy
    gen = torch.Generator().manual_seed(21)
    torch.manual_seed(21)
    actor, critic = perturb_bn(RefLayout(4), gen).to(DEV), perturb_bn(RefLayout(1), gen).to(DEV)
    net = DevicePolicy(actor, critic, precision=precision)

    def blob(module, n_out, apply_bn):
        folded = policy.fold(policy.parse(module, n_out)[0], apply_bn)
        return ops.policy_pack(torch.cat([p.reshape(-1) for Wb in folded for p in Wb]).float(), n_out, precision)

    def direct(boards):         # the reference's layout skips BatchNorm for a batch of one row
        bn = boards.shape[0] > 1
        return ops.policy_forward(boards, blob(actor, 4, bn), blob(critic, 1, bn), precision)
    return (net, direct, list(net.actor.plain.values()) + list(net.critic.plain.values()),
            list(net.actor.packed.values()) + list(net.critic.packed.values()))


def make_encoder(precision, module, cls_name, model, forward_name, pack_name):
    import g2048
    from g2048 import ops
    net = getattr(g2048, cls_name)(model.to(DEV), precision=precision)

    def direct(boards):
        fresh = getattr(ops, pack_name)(module.flatten(module.parse(model)), net.dim_ff, net.n_layers, precision)
        return getattr(ops, forward_name)(boards, fresh, net.dim_ff, net.n_layers, precision)
    return net, direct, [net.plain], [net.packed]


def make_tpolicy(precision):
    from g2048 import tpolicy
    torch.manual_seed(22)
    model = test_tpolicy_host.scale_heads(test_tpolicy_host.RefSpelling(32, 1).eval())
    return make_encoder(precision, tpolicy, "DeviceTransformerPolicy", model, "tpolicy_forward", "tpolicy_pack")


def make_qnet(precision):
    from g2048 import qnet
    return make_encoder(precision, qnet, "DeviceQNetwork", test_qnet_host.random_model(23, 32, 1), "qnet_forward", "qnet_pack")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("make", [make_policy, make_tpolicy, make_qnet])
def test_owned_buffers_in_place_refresh_and_the_direct_launch(make, precision):
    from g2048 import ops
    net, direct, plains, blobs = make(precision)
    boards = {n: ops.synth_boards(n, seed=31 + n, device=DEV) for n in SIZES}
    first, kept = {}, {}
    for n in SIZES:
        first[n] = as_tuple(net(boards[n]))
        kept[n] = [t.clone() for t in first[n]]
        want = as_tuple(direct(boards[n]))
        assert len(want) == len(first[n])
        for got, w in zip(first[n], want):                                       # (d) the direct launch on a freshly packed blob
            assert got.shape == w.shape and torch.equal(got, w), (n, got.shape)
    ptrs = {n: [t.data_ptr() for t in first[n]] for n in SIZES}
    assert len({p for n in SIZES for p in ptrs[n]}) == sum(len(v) for v in ptrs.values())      # (b) another N, other storage
    for n in SIZES:
        assert [t.data_ptr() for t in as_tuple(net(boards[n]))] == ptrs[n]       # (a) same N, same stream: the same storage
    torch.cuda.synchronize()
    for n in SIZES:
        for t, k in zip(first[n], kept[n]):                                      # (b) ... and no call with another N wrote into it
            assert torch.equal(t, k), n
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = as_tuple(net(boards[17]))
    side.synchronize()
    assert not set(t.data_ptr() for t in other) & set(ptrs[17])                  # (b) a second stream, other storage
    for t, k in zip(other, kept[17]):
        assert torch.equal(t, k)
    where = [t.data_ptr() for t in plains + blobs]
    before = [t.clone() for t in blobs]
    net.refresh()
    assert [t.data_ptr() for t in plains + blobs] == where                       # (c) refresh() writes in place
    for t, k in zip(blobs, before):
        assert torch.equal(t, k)                                                 # (unchanged weights pack to the same bytes)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_qnet_act_is_forward_plus_select(precision):
    from g2048 import ops
    net, _, _, _ = make_qnet(precision)
    for n in SIZES:
        boards = ops.synth_boards(n, seed=41 + n, device=DEV)
        exploit, q0 = net.act(boards)
        want_exploit, want_q = ops.qnet_forward(boards, net.packed, net.dim_ff, net.n_layers, precision, want_actions=True)
        assert torch.equal(exploit, want_exploit) and torch.equal(q0, want_q)
        exploit_at = exploit.data_ptr()
        actions, q = net.act(boards, epsilon=0.5, **KEYS)
        assert actions.data_ptr() == exploit_at and q.data_ptr() == q0.data_ptr() == net(boards).data_ptr()
        want, explored = ops.qnet_select_actions(want_q, boards, 0.5, actions=want_exploit.clone(), **KEYS)
        assert torch.equal(actions, want) and actions.dtype == torch.uint8 and actions.shape == (n,)
        again, _ = net.act(boards, epsilon=0.5, **KEYS)
        assert again.data_ptr() == exploit_at and torch.equal(again, want)
    assert 0 < int(explored.sum()) < SIZES[-1]                                   # at epsilon 0.5 some of 33 boards explore, some do not
