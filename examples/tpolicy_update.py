#!/usr/bin/env python3
"""A PPO update of the reference's transformer policy (models/transformer.py) with its loss, gradients and optimiser on the GPU.

    python examples/tpolicy_update.py [--envs 256] [--updates 5] [--epochs 3] [--dim-ff 2048] [--precision f32|bf16] [--lr 3e-4]
                                      [--grad-precision f32|bf16] [--optimizer device|torch] [--dropout P|module] [--dropout-seed S]
                                      [--collector single|fused|collect] [--steps 8]

A stock-torch module with the reference's layout, a VecGame2048 batch, one step of every env acted by
g2048.DeviceTransformerPolicy (the probabilities of one g2048_tpolicy_forward launch, PPOAgent.get_action's masked sampling), then
per update, with --optimizer device (the default): ONE net.update() call, which is net.advantages, --epochs rounds of
net.loss_and_grad and the device's NaN gate, clipping at 0.5 and Adam step on net.plain (g2048_tpolicy_adam_step), and one pack of
the acting blob at the end; a skipped epoch shows in net.opt_counters. With --optimizer torch the same update from its pieces and
stock torch: net.advantages (agents/ppo_agent.py:357-373 with this network's critic head) and --epochs rounds of
net.loss_and_grad (:378-400 on the two heads, eval mode: the forward with its activations kept, the loss head and the backward on
the device, the gradients landing in the views attach_grads() gave the module's parameters), clip_grad_norm_ at 0.5, a stock
torch.optim.Adam on the views attach_params() made of net.plain, and net.refresh() (which then only packs the acting blob again).
No gradient copy and no host synchronisation inside an update; the loss parts are read back once per update, to print them.
--envs is at most 1,024, the pass's limit. --dropout P (or "module" for the layers' own 0.1) makes the update the reference's: its
networks stay in training mode through PPOAgent.update(), so the advantage block's two critic forwards and every epoch's forward run
the encoder's four dropout sites, here with counter-RNG masks keyed by (--dropout-seed, net.dropout_index) and regenerated in the
backward pass; acting stays eval mode.
--collector single (the default) is the hand-written loop above: one step of every env, torch's masked_sample. --collector fused
and --collector collect take the experience from g2048.RolloutCollector(--envs, --steps, net, sampler=..., minibatches=True)
instead: per update one collect() of --steps steps (fused: a forward and a rollout step per env step, replayed from a graph;
collect: ONE g2048_tpolicy_collect launch), then sample(B, as_boards=True), B = min(1,024, --envs x --steps) distinct transitions
as the packed boards net.update() takes. The update packs the acting blob in place, so the next collect acts with the new weights.
The script shows that the pieces fit; it makes no claim about learning.
"""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "2048-using-reinforcement-learning_amd"))
import g2048

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=256)
ap.add_argument("--updates", type=int, default=5)
ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--dim-ff", type=int, default=2048)
ap.add_argument("--precision", choices=("f32", "bf16"), default="f32", help="of the acting blob; the gradient pass is --grad-precision's")
ap.add_argument("--grad-precision", choices=("f32", "bf16"), default="f32",
                help="bf16: every encoder layer's feed-forward products of the gradient pass on the bf16 matrix cores (not a rounding-level change)")
ap.add_argument("--lr", type=float, default=3e-4)
ap.add_argument("--optimizer", choices=("device", "torch"), default="device",
                help="device: net.update(), clipping and Adam in the library; torch: clip_grad_norm_ and torch.optim.Adam on attached views")
ap.add_argument("--dropout", default="0", help="a probability for the encoder's four dropout sites, or 'module' for the layers' own; 0: eval mode")
ap.add_argument("--dropout-seed", type=int, default=0)
ap.add_argument("--collector", choices=("single", "fused", "collect"), default="single",
                help="single: one env step by torch's masked_sample; fused / collect: g2048.RolloutCollector with that sampler")
ap.add_argument("--steps", type=int, default=8, help="with --collector fused / collect: env steps per collect")
a = ap.parse_args()
dropout = a.dropout if a.dropout == "module" else float(a.dropout)
if not 1 <= a.envs <= 1024:
    sys.exit("--envs must be 1 .. 1024: loss_and_grad takes at most 1,024 boards a call")


class TransformerModel(nn.Module):      # the reference's layout (models/transformer.py:4-40), stock torch, default init
    def __init__(self, dim_ff):
        super().__init__()
        self.embedding = nn.Linear(1, 64)
        layer = nn.TransformerEncoderLayer(d_model=64, nhead=4, dim_feedforward=dim_ff, batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=2)
        self.fc1, self.fc2 = nn.Linear(1024, 128), nn.Linear(128, 64)
        self.actor, self.critic = nn.Linear(64, 4), nn.Linear(64, 1)


dev, seed = torch.device("cuda"), 1
torch.manual_seed(0)
net = g2048.DeviceTransformerPolicy(TransformerModel(a.dim_ff).to(dev).eval(), precision=a.precision, dropout=dropout,
                                    dropout_seed=a.dropout_seed, grad_precision=a.grad_precision)
net.attach_params()                    # the module's parameters are views of net.plain from here on
if a.optimizer == "torch":
    net.attach_grads()                 # and their .grad views of net.grad
    optimizer = torch.optim.Adam(net.model.parameters(), lr=a.lr)
if a.collector == "single":
    env = g2048.VecGame2048(a.envs, device=dev, seed=seed)
    gen = torch.Generator(device=dev).manual_seed(seed)
else:
    if a.steps < 1:
        sys.exit("--steps must be at least 1")
    rc = g2048.RolloutCollector(a.envs, a.steps, net, device=dev, seed=seed, sampler=a.collector, minibatches=True)
    batch = min(1024, a.envs * a.steps)

for update in range(a.updates):
    if a.collector == "single":
        boards = env.boards.clone()
        probs, _ = net(boards)
        actions, old_log_probs = g2048.masked_sample(probs, g2048.ops.valid_moves(boards), generator=gen)
        next_boards, reward, done, _ = env.step(actions)
        next_boards, reward, dones = next_boards.clone(), reward.float().clone(), done.float()
        actions = actions.to(torch.int64)
    else:
        rc.collect()
        mb = rc.sample(batch, as_boards=True)      # states / next_states as packed boards
        boards, actions, old_log_probs, reward, next_boards, dones = (mb[k] for k in ("states", "actions", "old_log_probs", "rewards",
                                                                                     "next_states", "dones"))
    if a.optimizer == "device":
        rows, _ = net.update(boards, actions, old_log_probs, reward, next_boards, dones, epochs=a.epochs, lr=a.lr)
        losses = rows[-1]
    else:
        returns, advantages = net.advantages(boards, next_boards, reward, dones)
        for epoch in range(a.epochs):
            losses, _, _ = net.loss_and_grad(boards, actions, old_log_probs, advantages, returns)     # fills net.grad
            torch.nn.utils.clip_grad_norm_(net.model.parameters(), max_norm=0.5)
            optimizer.step()           # no zero_grad: the next call overwrites
            net.refresh()              # attached: packs the acting blob, nothing else
    loss, actor, value, entropy = losses.tolist()
    print("update %d: %d boards, last epoch's loss %.4f = actor %.4f + 0.4 x value %.4f - 0.05 x entropy %.4f; mean reward %.2f"
          % (update, boards.shape[0], loss, actor, value, entropy, float(reward.mean())))
    if a.collector == "single":
        fresh, _ = g2048.ops.reset(a.envs, seed, update + 1, 0, device=dev)
        env.load(torch.where(done[:, None], fresh, env.boards), torch.where(done, torch.zeros_like(env.scores), env.scores))
if a.collector != "single":
    print("collector %s: %d collects of %d envs x %d steps, %d transitions sampled per update" % (a.collector, a.updates, a.envs, a.steps, batch))
print("parameters attached: %s; %d floats of gradient in place" % (net.params_attached, net.grad.numel()))
print("dropout %s: %d training forwards, seed %d" % (net.dropout, net.dropout_index, net.dropout_seed))
if a.optimizer == "device":
    print("device optimizer: %d Adam steps applied, %d epochs skipped for a NaN loss, %d for a gradient that is not finite"
          % tuple(net.opt_counters.tolist()))
