#!/usr/bin/env python3
"""The data side of the hybrid agent's training loop (reference agents/hybrid.py:955-1074) entirely on the GPU.

    python examples/dqn_replay.py [--envs 4096] [--steps 200] [--capacity 200000] [--batch 256] [--every 4] [--dim-ff 2048] [--train]
                                  [--device-step] [--dropout 0.1 | module] [--collector legacy|fused|stepwise] [--collect-steps 16]

A VecGame2048 batch is played by DeviceQNetwork.act(epsilon=...) (DQNAgent.select_action); every step of every env is pushed
into a g2048.DeviceReplayBuffer (PrioritizedReplayBuffer.push); every --every steps a batch is sampled -- sample(), the float32
tensors train_step builds and its reward shaping, one call, no host round trip --, the Double-DQN targets come from
g2048.dqn_targets (:1041-1046: the online and the target network's batch forward on the next states, as the reference makes
it: one sequence of tokens that attend to each other, then argmax, gather and the target in one launch), the current Q from
online.forward_batch (:1038), and the Huber errors go back as the new priorities (:1050, :1063-1064). The batch forward is f32
only, so --precision bf16 applies to the acting network alone.
Without --train there is no optimiser here and no claim about learning; the script shows that the pieces fit and prints the rates.

--train runs the whole train_step (:955-1074): sample, targets, online.loss_and_grad (the forward with its activations kept, the
prioritised Huber loss and the backward pass on the device, the gradients landing in the views attach_grads() gave the module's
parameters), then stock torch for the elementwise rest -- clip_grad_norm_ at 10, AdamW(lr 1e-3, weight_decay 1e-4),
CosineAnnealingLR --, update_priorities(indices, td + 1e-5), online.refresh(), and the target network synchronised every 250
training steps. Still no claim about learning curves.

--train --dropout P (or --dropout module, the layers' own 0.1): the three forwards of train_step -- both networks' in dqn_targets and
the one loss_and_grad keeps -- run the encoder layers' four dropout sites live, as the reference's do (it never calls .eval()); the
online and the target network draw from different seeds. Acting stays eval mode. Without --dropout: eval mode throughout.

--collector fused | stepwise hands the acting side to g2048.DQNCollector (train_agent's loop, :1098-1127: the reference's reset rule
and its max_steps of 2000): `fused` plays --collect-steps moves of every env and writes their transitions into the ring in ONE kernel
launch, `stepwise` is the same function made of the older entry points, one env step at a time; the sample + update rounds that
fall into a chunk follow it. `legacy`, the default, is the loop below (play()) as it always was.

--train --device-step keeps that tail on the device too: attach_params() makes both modules views of their plain buffers,
online.adamw_step(g2048.cosine_lr(round)) is the clipping, the AdamW update and the re-pack in two launches plus the pack, and
target.sync_from(online) is the target update in one copy; the last gradient norm is printed at the end.
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "2048-using-reinforcement-learning_amd"))
import g2048

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--capacity", type=int, default=200000)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--every", type=int, default=4, help="env steps between two sample + update rounds")
ap.add_argument("--epsilon", type=float, default=0.2)
ap.add_argument("--dim-ff", type=int, default=2048)
ap.add_argument("--precision", choices=("f32", "bf16"), default="f32")
ap.add_argument("--train", action="store_true", help="the full train_step: loss_and_grad, clip, AdamW, cosine schedule, target sync")
ap.add_argument("--device-step", action="store_true", help="with --train: clipping, AdamW and the target sync on the device (adamw_step, sync_from)")
ap.add_argument("--dropout", default="0", help="with --train: a probability for the encoder layers' four dropout sites in the training forwards, or 'module'")
ap.add_argument("--collector", choices=("legacy", "fused", "stepwise"), default="legacy", help="who plays: the loop of this script, or g2048.DQNCollector")
ap.add_argument("--collect-steps", type=int, default=16, help="with --collector fused | stepwise: env steps per collect call")
a = ap.parse_args()
if a.device_step and not a.train:
    sys.exit("--device-step needs --train")
dropout = a.dropout if a.dropout == "module" else float(a.dropout)
if dropout != 0 and not a.train:
    sys.exit("--dropout needs --train")
if a.envs > a.capacity:
    sys.exit("--envs must not exceed --capacity: a push holds one transition per env")
if a.collector != "legacy" and (a.collect_steps < 1 or a.collect_steps * a.envs > a.capacity):
    sys.exit("--collect-steps x --envs must lie in 1 .. --capacity: a collect call holds that many transitions")


class HybridDQN(nn.Module):             # the reference's layout (agents/hybrid.py:700-727), stock torch, default init
    def __init__(self, dim_ff):
        super().__init__()
        self.cnn = nn.Sequential(nn.Conv2d(1, 32, kernel_size=2, stride=1, padding=1), nn.ReLU(),
                                 nn.Conv2d(32, 64, kernel_size=2, stride=1, padding=0), nn.ReLU())
        self.embedding = nn.Linear(1024, 128)
        self.transformer = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=128, nhead=8, dim_feedforward=dim_ff), 2,
                                                 enable_nested_tensor=False)
        self.fc = nn.Linear(128, 4)


dev, seed, gamma = torch.device("cuda"), 1, 0.99
torch.manual_seed(0)
online = g2048.DeviceQNetwork(HybridDQN(a.dim_ff).to(dev).eval(), dropout=dropout, dropout_seed=seed)
target = g2048.DeviceQNetwork(HybridDQN(a.dim_ff).to(dev).eval(), dropout=dropout, dropout_seed=seed + 1)     # its own masks
actor = online if a.precision == "f32" else g2048.DeviceQNetwork(online.model, precision=a.precision)     # the same module
env = g2048.VecGame2048(a.envs, device=dev, seed=seed)
buf = g2048.DeviceReplayBuffer(a.capacity, alpha=0.6, device=dev, seed=seed)
collector = g2048.DQNCollector(actor, buf, a.envs, seed=seed, device=dev) if a.collector != "legacy" else None
huber = nn.SmoothL1Loss(reduction="none")
TARGET_SYNC = 250
last_norm = None
if a.device_step:
    online.attach_params()             # both modules are their plain buffers from here on
    target.attach_params()
elif a.train:
    online.attach_grads()              # every parameter's .grad is a view into online.grad from here on
    optimizer = torch.optim.AdamW(online.model.parameters(), lr=1e-3, weight_decay=1e-4)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=10000, eta_min=1e-5)


def play(t):
    state = env.boards.clone()
    actions, _ = actor.act(state, epsilon=a.epsilon, seed=seed, step_index=t)
    nxt, reward, done, _ = env.step(actions)
    buf.push(state, actions, reward, nxt, env.flags)
    # finished games start over (the next state pushed above is the finished board, as the reference's loop stores it)
    fresh, _ = g2048.ops.reset(a.envs, seed, t + 1, 0, device=dev)
    env.load(torch.where(done[:, None], fresh, nxt), torch.where(done, torch.zeros_like(env.scores), env.scores))


def learn(round_index):
    beta = 0.4 + 0.6 * min(round_index / 1000.0, 1.0)
    (states, actions, rewards, next_states, dones), indices, weights, shaped = buf.sample(a.batch, beta=beta)
    boards, next_boards = buf.boards(indices)              # the same batch as uint8 codes, the form DeviceQNetwork reads
    targets, _ = g2048.dqn_targets(online, target, next_boards, shaped, dones, gamma, training=a.train)
    if a.train:
        return train(round_index, boards, actions, targets, weights, indices)
    q = online.forward_batch(boards).gather(1, actions.unsqueeze(1)).squeeze(1)
    td = huber(q, targets)
    buf.update_priorities(indices, td)
    return (weights * td).mean()


def train(round_index, boards, actions, targets, weights, indices):
    loss, td, _ = online.loss_and_grad(boards, actions, targets, weights)             # :1038, :1049-1055; fills online.grad
    if a.device_step:
        return device_step(round_index, loss, td, indices)
    torch.nn.utils.clip_grad_norm_(online.model.parameters(), max_norm=10.0)
    optimizer.step()                                                                  # no zero_grad: the next call overwrites
    scheduler.step()
    buf.update_priorities(indices, td)                                                # adds the reference's 1e-5 itself
    online.refresh()
    if actor is not online:
        actor.refresh()
    if (round_index + 1) % TARGET_SYNC == 0:
        target.model.load_state_dict(online.model.state_dict())
        target.refresh()
    return loss


def device_step(round_index, loss, td, indices):
    global last_norm
    last_norm = online.adamw_step(g2048.cosine_lr(min(round_index, 10000), t_max=10000, eta_min=1e-5), max_norm=10.0)   # the schedule above
    buf.update_priorities(indices, td)
    if actor is not online:
        actor.refresh()
    if (round_index + 1) % TARGET_SYNC == 0:
        target.sync_from(online)
    return loss


def run_collected(steps, t0):
    rounds, loss, t = 0, None, t0
    while t < t0 + steps:
        k = min(a.collect_steps, t0 + steps - t)
        collector.collect(k, a.epsilon, fused=a.collector == "fused")
        for u in range(t, t + k):
            if len(buf) >= a.batch and (u + 1) % a.every == 0:
                loss = learn(rounds)
                rounds += 1
        t += k
    return rounds, loss


def run(steps, t0):
    if collector is not None:
        return run_collected(steps, t0)
    rounds, loss = 0, None
    for t in range(t0, t0 + steps):
        play(t)
        if len(buf) >= a.batch and (t + 1) % a.every == 0:
            loss = learn(rounds)
            rounds += 1
    return rounds, loss


warm = min(a.steps, 2 * a.every)
run(warm, 0)
torch.cuda.synchronize()
start = time.perf_counter()
rounds, loss = run(a.steps, warm)
torch.cuda.synchronize()
dt = time.perf_counter() - start
print("%d envs x %d steps: %d transitions pushed in %.3f s = %.3g transitions/s, with %d sample + update rounds of %d (%.3g rounds/s)"
      % (a.envs, a.steps, a.envs * a.steps, dt, a.envs * a.steps / dt, rounds, a.batch, rounds / dt))
prio = buf.logical_priorities()
print("buffer: %d of %d entries, priorities %.3g .. %.3g, last weighted Huber loss %s"
      % (len(buf), a.capacity, float(prio.min()), float(prio.max()), "%.4g" % float(loss) if loss is not None else "none"))
if a.train:
    print("dropout %s: %d training forwards of the online network, %d of the target network"
          % (online.dropout, online.dropout_index, target.dropout_index))
if last_norm is not None:
    print("device step: %d updates, last gradient norm before clipping %.4g" % (online.opt_step, float(last_norm)))
