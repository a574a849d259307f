"""The hybrid agent's PrioritizedReplayBuffer (reference agents/hybrid.py:730-765) resident on the device.

    buf = g2048.DeviceReplayBuffer(200_000, alpha=0.6)
    buf.push(boards, actions, rewards, next_boards, flags)            # every env of a batched step
    (states, actions, rewards, next_states, dones), indices, weights, shaped_rewards = buf.sample(256, beta=0.4)
    ...                                                                # the caller's networks, loss and optimiser
    buf.update_priorities(indices, td_errors)

sample() also does what DQNAgent.train_step does to its batch before the networks see it (:961-969 the float32 tensors of tile
values, :971-1034 the reward shaping), so nothing of a training step but the gradient work is left to the caller. Nothing here
synchronises: the ring's size, its head and the sample counter are Python integers, every call is a few launches on torch's
current stream. (Capturing the calls in a hipGraph is not supported: size and head are launch arguments.)
"""
import torch

from . import ops


class DeviceReplayBuffer:
    def __init__(self, capacity, alpha=0.6, device="cuda", seed=0x2048):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("g2048: capacity must be at least 1")
        self.capacity, self.alpha, self.seed = capacity, float(alpha), int(seed)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("g2048: DeviceReplayBuffer needs a ROCm device (got %s); there is no CPU path" % self.device)
        dev = self.device
        self.states = torch.zeros((capacity, 16), dtype=torch.uint8, device=dev)
        self.next_states = torch.zeros((capacity, 16), dtype=torch.uint8, device=dev)
        self.actions = torch.zeros(capacity, dtype=torch.uint8, device=dev)
        self.rewards = torch.zeros(capacity, dtype=torch.float32, device=dev)
        self.dones = torch.zeros(capacity, dtype=torch.uint8, device=dev)
        self.priorities = torch.zeros(capacity, dtype=torch.float32, device=dev)
        self.size = 0                      # live entries
        self.head = 0                      # physical slot of the oldest entry (logical index 0, the reference's deque index 0)
        self.samples = 0                   # sample() calls so far: the index of the next call's counter draws
        self._sample_ws = torch.empty((ops.per_sample_workspace_bytes(capacity) + 7) // 8, dtype=torch.float64, device=dev)
        self._update_ws = torch.empty((ops.per_update_workspace_bytes(capacity) + 7) // 8, dtype=torch.float64, device=dev)

    def __len__(self):
        return self.size

    def _ring(self):
        return self.states, self.next_states, self.actions, self.rewards, self.dones, self.priorities

    def push(self, boards, actions, rewards, next_boards, flags):
        """One push (:736-740) per row, in order: boards / next_boards uint8 (m,16) codes (the next states before any auto-reset),
        actions uint8, rewards float32 or float64, flags uint8 (bit 0 = done, as the step kernels write them). m <= capacity."""
        self.size, self.head = ops.per_push(*self._ring(), self.size, self.head, boards, actions, rewards, next_boards, flags,
                                            workspace=self._update_ws)

    def sample(self, batch_size, beta=0.4, u=None, out=None, want_probs=False):
        """sample (:742-757) and the head of train_step: ((states, actions, rewards, next_states, dones), indices, weights,
        shaped_rewards), every tensor on the device (states float32 (batch,16) tile values, actions int64, dones float32).
        u: float64 (batch,) uniforms to use instead of the buffer's own counter draws. With want_probs the sampling
        probabilities float32 (len,) come fifth. Fewer entries than batch_size is an error: train_step does not sample then."""
        if self.size < int(batch_size):
            raise ValueError("g2048: the buffer holds %d transitions, fewer than the batch of %d" % (self.size, int(batch_size)))
        r = ops.per_sample(*self._ring(), self.size, self.head, self.alpha, beta, batch_size, seed=self.seed, sample_index=self.samples,
                           u=u, workspace=self._sample_ws, out=out, want_probs=want_probs)
        self.samples += 1
        res = ((r["states"], r["actions"], r["rewards"], r["next_states"], r["dones"]), r["indices"], r["weights"], r["shaped"])
        return res + (r["probs"],) if want_probs else res

    def update_priorities(self, indices, td_errors):
        """update_priorities(indices, td_errors + 1e-5) as train_step calls it (:1063-1064): indices int64 as sample returned
        them, td_errors float32."""
        ops.per_update_priorities(self.priorities, self.size, self.head, indices, td_errors, workspace=self._update_ws)

    def boards(self, indices):
        """(states, next_states) of the entries `indices` (as sample returned them) as uint8 (batch,16) codes: the form
        DeviceQNetwork reads. Valid until the next push."""
        slots = (indices + self.head) % self.capacity
        return self.states[slots], self.next_states[slots]

    def logical_priorities(self):
        """The live priorities in the reference's deque order (a copy)."""
        order = (torch.arange(self.size, device=self.device) + self.head) % self.capacity
        return self.priorities[order]
