"""The acting half of the hybrid agent's train_agent (reference agents/hybrid.py:1089-1127) on the device: n environments played by
a DeviceQNetwork with DQNAgent.select_action, every transition written into a DeviceReplayBuffer.

    net = g2048.DeviceQNetwork(model)
    buf = g2048.DeviceReplayBuffer(200_000)
    col = g2048.DQNCollector(net, buf, n_envs=4096, seed=1)
    col.prefill(1000)                                                  # train_agent's warm-up: one random move of fresh boards
    flags, indices = col.collect(16, epsilon=g2048.dqn_epsilon(t))     # 16 moves of every env: ONE kernel launch, into the ring
    ...                                                                # buf.sample / dqn_targets / net.loss_and_grad / net.adamw_step

collect(fused=True) is one g2048_qnet_collect call (include/g2048_collect.h): at most three stream operations for steps x n_envs
transitions. collect(fused=False) is the same function made of the entry points that were there before it, one env step at a
time -- net.act / net.act_beam, ops.step without and with auto-reset, buffer.push --, about a dozen stream operations per env
step: the yardstick of the tests and of tools/qnet_collect_rate.py. Both leave the ring, the environments and the flags the
same, bit for bit.

An episode ends when the step says done, or, as train_agent's `step < max_steps` ends it, when it reaches max_episode_steps
moves; the stored done stays 0 in the second case. Either way the environment goes on from the board ops.step(auto_reset=True)
gives a finished board: fresh_board of the EPISODE-domain draws of that step index and env id. The stepwise path gets that board
for a truncated episode from the same entry point, by stepping a board that has no move left with the env's step index and id.
Nothing here synchronises: the step index, the ring's size and head are Python integers. (Capturing collect in a hipGraph is
not supported: size and head are launch arguments.)
"""
import torch

from . import ops
from ._lib import FLAG_DONE

# a full board without two equal neighbours: every move is invalid and leaves it finished, so ops.step(auto_reset=True) answers
# with the fresh board of the step index and id it is given
_DEAD_BOARD = (1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1)


class DQNCollector:
    """n_envs environments of net (a DeviceQNetwork) feeding buffer (a DeviceReplayBuffer). boards uint8 (n,16), scores int32,
    moves int32 (the episodes' move counts) and step_index (the index of the next env step's draws, which counts on over the
    calls) are the collector's; env i has id id_base + i. max_episode_steps: train_agent's max_steps, 0 = no cap."""

    def __init__(self, net, buffer, n_envs, seed=0x2048, id_base=0, max_episode_steps=2000, device="cuda"):
        n_envs, max_episode_steps = int(n_envs), int(max_episode_steps)
        if n_envs < 1:
            raise ValueError("g2048: n_envs must be at least 1")
        if max_episode_steps < 0:
            raise ValueError("g2048: max_episode_steps must be 0 (no cap) or positive")
        self.net, self.buffer, self.n = net, buffer, n_envs
        self.seed, self.id_base, self.max_episode_steps = int(seed), int(id_base), max_episode_steps
        self.device = torch.device(device)
        self.boards, self.scores = ops.reset(n_envs, self.seed, 0, self.id_base, device=self.device)
        self.moves = torch.zeros(n_envs, dtype=torch.int32, device=self.device)
        self.step_index = 0
        self._workspace = torch.empty((ops.qnet_collect_workspace_bytes(n_envs) + 7) // 8, dtype=torch.float64, device=self.device)
        self._dead = None                  # the stepwise path's finished boards, made on first use

    def _new_indices(self, m):
        """The logical indices of the m newest entries."""
        return torch.arange(self.buffer.size - m, self.buffer.size, dtype=torch.int64, device=self.device)

    def collect(self, steps, epsilon, use_beam_search=False, beam_width=15, search_depth=30, threshold=64, fused=True):
        """`steps` moves of every env, the transitions pushed in the order (step, env). Returns (flags uint8 (steps, n): every
        step's flags byte, indices int64 (steps * n,): the new entries' logical indices in the buffer, valid until the next
        push). use_beam_search: select_action with the reference's beam search at (beam_width, search_depth, threshold); fused
        needs search_depth >= 2 then."""
        steps = int(steps)
        if steps < 1:
            raise ValueError("g2048: steps must be at least 1")
        if steps * self.n > self.buffer.capacity:
            raise ValueError("g2048: steps x n_envs = %d x %d transitions exceed the buffer's capacity of %d"
                             % (steps, self.n, self.buffer.capacity))
        beam = (int(beam_width), int(search_depth), int(threshold)) if use_beam_search else None
        if fused:
            flags = self._collect_fused(steps, float(epsilon), beam)
        else:
            flags = torch.empty((steps, self.n), dtype=torch.uint8, device=self.device)
            for t in range(steps):
                self._step(float(epsilon), beam, flags[t])
        return flags, self._new_indices(steps * self.n)

    def _collect_fused(self, steps, epsilon, beam):
        buf, net = self.buffer, self.net
        width, depth, threshold = beam if beam else (0, 30, 64)
        buf.size, buf.head, flags = ops.qnet_collect(
            self.boards, self.scores, self.moves, net.packed, net.dim_ff, net.n_layers, *buf._ring(), buf.size, buf.head, steps,
            precision=net.precision, epsilon=epsilon, beam_width=width, search_depth=depth, threshold=threshold, seed=self.seed,
            step_index0=self.step_index, id_base=self.id_base, max_episode_steps=self.max_episode_steps, workspace=self._workspace)
        self.step_index += steps
        return flags

    def _step(self, epsilon, beam, flags_out):
        """One env step of every env with the entry points of g2048.h alone."""
        net, seed, index, base = self.net, self.seed, self.step_index, self.id_base
        state = self.boards
        if beam:
            actions, _ = net.act_beam(state, epsilon, seed, index, base, beam_width=beam[0], search_depth=beam[1], beam_search_threshold=beam[2])
        else:
            actions, _ = net.act(state, epsilon, seed, index, base)
        nxt, reward, _ = ops.step(state, actions, self.scores.clone(), seed, index, base, flags=flags_out)       # what is remembered
        cont, _, _ = ops.step(state, actions, self.scores, seed, index, base, auto_reset=True)                  # what is played on
        self.buffer.push(state, actions, reward, nxt, flags_out)
        self.moves += 1
        ended = (flags_out & FLAG_DONE) != 0
        if self.max_episode_steps > 0:
            if self._dead is None:
                self._dead = torch.tensor(_DEAD_BOARD, dtype=torch.uint8, device=self.device).repeat(self.n, 1)
            fresh, _, _ = ops.step(self._dead, actions, torch.zeros_like(self.scores), seed, index, base, auto_reset=True)
            truncated = (self.moves >= self.max_episode_steps) & ~ended
            cont = torch.where(truncated[:, None], fresh, cont)
            self.scores = torch.where(truncated, torch.zeros_like(self.scores), self.scores)
            ended = ended | truncated
        self.moves = torch.where(ended, torch.zeros_like(self.moves), self.moves)
        self.boards = cont
        self.step_index += 1

    def prefill(self, m, epoch=1):
        """train_agent's buffer warm-up (hybrid.py:1089-1096): m fresh boards (ops.reset at `epoch`, ids id_base ..), one uniformly
        random action each -- unmasked, the draws of ops.synth_actions(seed, step_index 0) --, pushed. The collector's own
        environments and step index are not touched. Returns the new entries' logical indices."""
        m = int(m)
        if m > self.buffer.capacity:
            raise ValueError("g2048: %d transitions exceed the buffer's capacity of %d" % (m, self.buffer.capacity))
        boards, scores = ops.reset(m, self.seed, epoch, self.id_base, device=self.device)
        actions = ops.synth_actions(m, self.seed, 0, self.id_base, device=self.device)
        nxt, reward, flags = ops.step(boards, None, scores, self.seed, 0, self.id_base)
        self.buffer.push(boards, actions, reward, nxt, flags)
        return self._new_indices(m)
