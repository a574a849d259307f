"""Tensor-in / tensor-out wrappers of the C-ABI (one function per entry point of include/g2048.h).

Boards are torch.uint8 tensors of shape (n, 16) holding log2 codes (0 = empty), on a ROCm device.
Every call is enqueued on torch's current stream of the boards' device and returns immediately.
"""
import ctypes as C

import torch

from . import _lib as L


def _dev(t):
    return t.device


class KeyBlock:
    """Device-resident per-move RNG keys (include/g2048.h, "graph-replayable loops"). `advance()` enqueues the
    one-thread kernel that derives the keys of move `counter` and increments the counter; the ops below accept
    `keyblock=` instead of a host step index, which makes a captured hipGraph of one move replayable."""

    def __init__(self, seed, start=0, device="cuda"):
        self.seed = int(seed)
        self.device = torch.device(device)
        self.words = torch.zeros(L.KEYBLOCK_WORDS, dtype=torch.int32, device=self.device)
        self.counter = torch.full((1,), int(start), dtype=torch.int64, device=self.device)

    def advance(self):
        L.call(self.device, L.lib().g2048_keys_advance, self.words.data_ptr(), self.counter.data_ptr(), L.u64(self.seed),
               L.stream_ptr(self.device))
        return self


def _require_scores(scores):
    """scores are 32-bit on the device (the ABI's uint32); torch code usually holds them as int32."""
    L.require_device_tensor(scores, torch.uint32 if scores.dtype == torch.uint32 else torch.int32, None, "scores")


def _output(t, n, dtype, tail, name, device):
    """The output tensor `name` of n rows: allocated when t is None, else required to be a device tensor of `dtype` and, unless
    `tail` is None, of shape (n, *tail)."""
    if t is None:
        return torch.empty((n,) + tuple(tail or ()), dtype=dtype, device=device)
    L.require_device_tensor(t, dtype, tail, name)
    if tail is not None and t.shape[0] != n:
        raise ValueError("g2048: %s must have n %s" % (name, "rows" if tail else "entries"))
    return t


def _workspace(workspace, nb, dev):
    """The workspace of a call that needs nb bytes: allocated when None, else required to be a uint8 device tensor that holds them."""
    if workspace is None:
        workspace = torch.empty(nb, dtype=torch.uint8, device=dev)
    L.require_device_tensor(workspace, torch.uint8, None, "workspace")
    if workspace.numel() < nb:
        raise ValueError("g2048: workspace must hold at least %d bytes" % nb)
    return workspace


def _float_output(t, shape, name, dev):
    """The small float32 output `name` of an optimiser step, () or (2,): allocated when None, else required to hold as many."""
    if t is None:
        t = torch.empty(shape, dtype=torch.float32, device=dev)
    L.require_device_tensor(t, torch.float32, None, name)
    if t.numel() != (2 if shape else 1):
        raise ValueError("g2048: %s must hold %s float32" % (name, "two" if shape else "one"))
    return t


def _flat_plain(plain, floats):
    """plain: a flat float32 device tensor of `floats` parameters."""
    L.require_device_tensor(plain, torch.float32, None, "plain")
    if plain.dim() != 1 or plain.numel() != floats:
        raise ValueError("g2048: plain must be a flat float32 tensor of %d parameters" % floats)


def _grad_output(grad, floats, dev):
    """grad as given, or allocated: a flat float32 device tensor of `floats` floats."""
    if grad is None:
        grad = torch.empty(floats, dtype=torch.float32, device=dev)
    L.require_device_tensor(grad, torch.float32, None, "grad")
    if grad.dim() != 1 or grad.numel() != floats:
        raise ValueError("g2048: grad must be a flat float32 tensor of %d floats" % floats)
    return grad


def _sized(nb, message, *values):
    """A size query's bytes; 0 is the library's refusal of the arguments: ValueError(message % values)."""
    if nb == 0:
        raise ValueError(message % values)
    return nb


def _step_buffers(buffers):
    """The flat float32 buffers of an optimiser step, (name, tensor, floats) each: dtype and length of ALL of them before any
    device, since such a mistake reads the same everywhere; then every one on a device, and on the first one's, which is returned."""
    for name, t, floats in buffers:
        if not isinstance(t, torch.Tensor):
            raise TypeError("g2048: %s must be a torch.Tensor" % name)
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != floats:
            raise (TypeError if t.dtype != torch.float32 else ValueError)(
                "g2048: %s must be a flat float32 tensor of %d floats (got %s %s)" % (name, floats, t.dtype, tuple(t.shape)))
    first, dev = buffers[0][0], buffers[0][1].device
    for name, t, _ in buffers:
        L.require_device_tensor(t, torch.float32, None, name)
        if t.device != dev:
            raise ValueError("g2048: %s on %s, %s on %s" % (name, t.device, first, dev))
    return dev


def _step_counters(counters, count):
    L.require_device_tensor(counters, torch.int64, None, "counters")
    if counters.dim() != 1 or counters.numel() != count:
        raise ValueError("g2048: counters must be an int64 tensor of %d" % count)


def _gate_losses(losses):
    """The optional float32 tensor whose first element is the loss an optimiser step checks for NaN."""
    if losses is not None:
        L.require_device_tensor(losses, torch.float32, None, "losses")
        if losses.numel() < 1:
            raise ValueError("g2048: losses must hold at least one float32")


def step(boards, actions, scores, seed, step_index, id_base=0, out=None, reward=None, flags=None,
         reward_f64=False, auto_reset=False, tune=0, keyblock=None, noop_actions=False):
    """Game2048Env.step for every board (reference environment/game_2048.py:170-210).

    scores (uint32) is updated in place. Returns (boards_out, reward, flags); flags bit0 = done,
    bit1 = valid move, bits 3..7 = max log2 code. `out` may be `boards` for an in-place step.
    actions=None: random playout, the kernel draws the uniform actions synth_actions(seed, step_index) would give.
    noop_actions: action values above 3 move nothing (an invalid move), as in the reference; default: low two bits count."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    n = boards.shape[0]
    random_actions = actions is None
    if random_actions:
        if keyblock is not None:
            raise ValueError("g2048: random actions need the scalar (seed, step_index) form")
        actions = boards        # placeholder for the length check below; the pointer passed is NULL
    else:
        L.require_device_tensor(actions, torch.uint8, None, "actions")
    _require_scores(scores)
    if actions.shape[0] != n or scores.shape[0] != n:
        raise ValueError("g2048: actions/scores length must equal the number of boards")
    dev = _dev(boards)
    if out is None:
        out = torch.empty_like(boards)
    rdt = torch.float64 if reward_f64 else torch.float32
    if reward is None:
        reward = torch.empty(n, dtype=rdt, device=dev)
    if flags is None:
        flags = torch.empty(n, dtype=torch.uint8, device=dev)
    L.require_device_tensor(out, torch.uint8, (16,), "out")
    L.require_device_tensor(reward, rdt, None, "reward")
    L.require_device_tensor(flags, torch.uint8, None, "flags")
    opts = ((L.STEP_REWARD_F64 if reward_f64 else 0) | (L.STEP_AUTO_RESET if auto_reset else 0) |
            (L.STEP_RANDOM_ACTIONS if random_actions else 0) | (L.STEP_NOOP_ACTIONS if noop_actions else 0) | ((int(tune) & 3) << 8))
    act_ptr = None if random_actions else actions.data_ptr()
    if keyblock is not None:        # keys (and so seed / step index) come from the device key block
        L.call(dev, L.lib().g2048_step_dyn, boards.data_ptr(), act_ptr, out.data_ptr(), scores.data_ptr(),
               reward.data_ptr(), flags.data_ptr(), keyblock.words.data_ptr(), L.u64(id_base), n, opts, L.stream_ptr(dev))
    else:
        L.call(dev, L.lib().g2048_step, boards.data_ptr(), act_ptr, out.data_ptr(), scores.data_ptr(),
               reward.data_ptr(), flags.data_ptr(), L.u64(seed), L.u64(step_index), L.u64(id_base), n, opts,
               L.stream_ptr(dev))
    return out, reward, flags


class PreparedStep:
    """g2048_step with everything but the step index bound and checked ONCE: calling it costs one ctypes call of three
    arguments (g2048_step_packed on the block g2048_step_pack filled) instead of the tensor checks of `step`, so a host loop
    of back-to-back steps stays ahead of the GPU even at ~9 us per step. Same semantics as `step(..., out=, reward=, flags=)`
    with explicit actions. What g2048_step_pack refuses as more than one plain launch (a board-id range that crosses a
    multiple of 2^32) keeps going through g2048_step, twelve arguments a call."""

    def __init__(self, boards, actions, scores, seed, id_base=0, *, out, reward, flags, auto_reset=False, tune=0):
        step(boards, actions, scores, seed, 0, id_base, out=out, reward=reward, flags=flags,
             reward_f64=reward.dtype == torch.float64, auto_reset=auto_reset, tune=tune)        # validates everything (and runs once)
        self._keep = (boards, actions, scores, out, reward, flags)
        self.device = boards.device
        opts = ((L.STEP_REWARD_F64 if reward.dtype == torch.float64 else 0) | (L.STEP_AUTO_RESET if auto_reset else 0) |
                ((int(tune) & 3) << 8))
        head = (boards.data_ptr(), actions.data_ptr(), out.data_ptr(), scores.data_ptr(), reward.data_ptr(), flags.data_ptr(),
                L.u64(seed))
        tail = (L.u64(id_base), boards.shape[0], opts)
        self._block = (L.C.c_uint64 * (L.STEP_CALL_BYTES // 8))()
        self._call = L.C.addressof(self._block)
        self.packed = L.lib().g2048_step_pack(*head, *tail, self._call) == L.OK
        if self.packed:
            self._fn = L.lib().g2048_step_packed
        else:
            self._fn, self._head, self._tail = L.lib().g2048_step, head, tail

    def __call__(self, step_index, stream_ptr=None):
        if stream_ptr is None:
            stream_ptr = torch.cuda.current_stream(self.device).cuda_stream
        if self.packed:
            rc = self._fn(self._call, int(step_index), stream_ptr)
        else:
            rc = self._fn(*self._head, int(step_index), *self._tail, stream_ptr)
        if rc != L.OK:
            L.check(rc)


class StepChains:
    """Launch form for independent sub-batches ("chains") of one batch of boards: contiguous slices of whole kernel blocks,
    chain 0 on the caller's stream, chains 1..C-1 on side streams of their own. A chain's launches are ordered only behind
    that chain's earlier launches, so one chain's launch head and drain overlap the others' arithmetic -- what a single
    launch per step cannot do. Boards are independent and every draw is keyed by the global board id, so the
    results are the single launch's bit for bit. This object only does the stream bookkeeping:

        sc = StepChains(n, 2, device)
        sc.fork()                                  # side streams wait for the current stream's work so far
        for t in range(K):
            for c, (lo, hi) in enumerate(sc.bounds):
                with torch.cuda.stream(sc.stream(c)): ops.step(boards[lo:hi], ..., id_base + lo, ...)
        sc.join()                                  # the current stream waits for every chain

    Inside a hipGraph capture the same calls become one graph with C parallel branches. No host synchronisation anywhere."""

    ALIGN = 256          # a chain owns whole blocks of the step kernel, and 16-byte aligned slices of every per-board array

    def __init__(self, n, chains, device="cuda"):
        n, chains = int(n), int(chains)
        if chains < 1:
            raise ValueError("g2048: chains must be at least 1")
        self.device = torch.device(device)
        per = -(-max(n, 1) // chains)
        per = -(-per // self.ALIGN) * self.ALIGN
        self.bounds = [(lo, min(lo + per, n)) for lo in range(0, max(n, 1), per)]       # fewer than `chains` slices for a small n
        self._side = None
        self._events = None
        self._open_on = None        # the stream the open chains were forked from; None = joined
        self._held = []             # inputs of open chains, kept alive until the join

    def __len__(self):
        return len(self.bounds)

    @property
    def is_open(self):
        return self._open_on is not None

    def keep_alive(self, *tensors):
        """Side streams use these tensors: should they be freed with chains open, the allocator waits for the side streams."""
        if self._side is None:
            self._side = [torch.cuda.Stream(device=self.device) for _ in self.bounds[1:]]
        for t in tensors:
            for s in self._side:
                t.record_stream(s)

    def hold(self, tensor):
        self._held.append(tensor)

    def fork(self):
        """Open the chains on the current stream (no-op if they are open on it already). Returns the current stream."""
        cur = torch.cuda.current_stream(self.device)
        if self._open_on is not None:
            if self._open_on == cur:
                return cur
            self.join()             # the caller switched streams with chains open: close them where they were opened
        if self._side is None:
            self._side = [torch.cuda.Stream(device=self.device) for _ in self.bounds[1:]]
        self._order(cur, self._side)
        self._open_on = cur
        return cur

    def _order(self, first, then):
        """Every stream of `then` waits for what `first` holds now -- with events this object keeps (Stream.wait_stream makes a
        new one per call: ~10 us of host time each, which a fork + join per step pays twice)."""
        if self._events is None:
            self._events = [torch.cuda.Event() for _ in range(1 + len(self.bounds))]
        if isinstance(then, list):
            ev = self._events[0]
            ev.record(first)
            for s in then:
                s.wait_event(ev)
        else:                       # `first` is a list here: `then` waits for each of them
            for k, s in enumerate(first):
                ev = self._events[1 + k]
                ev.record(s)
                then.wait_event(ev)

    def stream(self, c):
        """The stream chain c launches on (valid between fork() and join())."""
        return self._open_on if c == 0 else self._side[c - 1]

    def fence(self):
        """Open chains wait for everything queued on the current stream so far (inputs produced after the fork)."""
        if self._open_on is not None:
            self._order(torch.cuda.current_stream(self.device), self._side)

    def join(self):
        """The stream the chains were opened on waits for every chain's last launch. No-op when nothing is open."""
        if self._open_on is not None:
            self._order(self._side, self._open_on)
            self._open_on = None
            self._held.clear()


def step_many(boards, scores, seed, step_index0, steps, id_base=0, out=None, flags=None, reward_stream=None,
              flags_stream=None, episodes=None, reward_f64=False, auto_reset=False, want_rewards=False, want_flags=False,
              want_episodes=False, actions=None):
    """`steps` consecutive steps of every board in ONE launch (g2048_step_many): step t equals
    `step(boards, actions[t] or None, scores, seed, step_index0 + t, id_base, auto_reset=...)` bit for bit, but the boards stay
    in registers between the steps. actions=None: random playout (uniform actions drawn in the kernel); else a uint8 (steps, n)
    tensor of explicit actions. scores is updated in place; `out` may be `boards`. Returns (boards_out, flags_last,
    reward_stream or None, flags_stream or None, episodes or None); the streams are (steps, n) tensors, allocated when want_*
    is set."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    n, steps = boards.shape[0], int(steps)
    if steps < 1:
        raise ValueError("g2048: steps must be at least 1")
    if actions is not None:
        L.require_device_tensor(actions, torch.uint8, None, "actions")
        if tuple(actions.shape) != (steps, n):
            raise ValueError("g2048: actions must have shape (steps, n)")
    _require_scores(scores)
    if scores.shape[0] != n:
        raise ValueError("g2048: scores length must equal the number of boards")
    dev = _dev(boards)
    if out is None:
        out = torch.empty_like(boards)
    if flags is None:
        flags = torch.empty(n, dtype=torch.uint8, device=dev)
    rdt = torch.float64 if reward_f64 else torch.float32
    if reward_stream is None and want_rewards:
        reward_stream = torch.empty((steps, n), dtype=rdt, device=dev)
    if flags_stream is None and want_flags:
        flags_stream = torch.empty((steps, n), dtype=torch.uint8, device=dev)
    if episodes is None and want_episodes:
        episodes = torch.empty(n, dtype=torch.int32, device=dev)
    L.require_device_tensor(out, torch.uint8, (16,), "out")
    L.require_device_tensor(flags, torch.uint8, None, "flags")
    for t, dt, name in ((reward_stream, rdt, "reward_stream"), (flags_stream, torch.uint8, "flags_stream")):
        if t is not None:
            L.require_device_tensor(t, dt, None, name)
            if tuple(t.shape) != (steps, n):
                raise ValueError("g2048: %s must have shape (steps, n)" % name)
    if episodes is not None:
        L.require_device_tensor(episodes, torch.int32, None, "episodes")
    opts = ((L.STEP_RANDOM_ACTIONS if actions is None else 0) | (L.STEP_REWARD_F64 if reward_f64 else 0) |
            (L.STEP_AUTO_RESET if auto_reset else 0))
    L.call(dev, L.lib().g2048_step_many, boards.data_ptr(), None if actions is None else actions.data_ptr(), out.data_ptr(),
           scores.data_ptr(),
           None if reward_stream is None else reward_stream.data_ptr(), None if flags_stream is None else flags_stream.data_ptr(),
           flags.data_ptr(), None if episodes is None else episodes.data_ptr(), L.u64(seed), L.u64(step_index0), steps,
           L.u64(id_base), n, opts, L.stream_ptr(dev))
    return out, flags, reward_stream, flags_stream, episodes


def reset(n, seed, epoch=0, id_base=0, device="cuda", boards=None, scores=None):
    """Game2048Env.reset for n boards (environment/game_2048.py:29-48). Returns (boards, scores)."""
    dev = torch.device(device) if boards is None else boards.device
    if boards is None:
        boards = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    if scores is None:
        scores = torch.empty(n, dtype=torch.int32, device=dev)
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _require_scores(scores)
    L.call(dev, L.lib().g2048_reset, boards.data_ptr(), scores.data_ptr(), L.u64(seed), L.u64(epoch), L.u64(id_base),
                                boards.shape[0], L.stream_ptr(dev))
    return boards, scores


def valid_moves(boards, agent_semantics=False, out=None):
    """4-bit masks (bit a = action a valid). Env semantics (game_2048.py:69-95) or the beam agent's own
    (_check_valid_moves, beam_search_agent.py:183-192 -- differs on DOWN)."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    out = _output(out, boards.shape[0], torch.uint8, None, "out", boards.device)
    L.call(boards.device, L.lib().g2048_valid_moves, boards.data_ptr(), out.data_ptr(), boards.shape[0],
                                      L.VALID_AGENT if agent_semantics else L.VALID_ENV, L.stream_ptr(boards.device))
    return out


def evaluate(boards, kind, phase=None, out=None):
    """Board heuristics in f64: L.EVAL_FAST / EVAL_FULL (phase uint8 per board or None) /
    EVAL_PPO_HEURISTIC / EVAL_MONO_*."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    if phase is not None:
        L.require_device_tensor(phase, torch.uint8, None, "phase")
        if phase.shape[0] != boards.shape[0]:
            raise ValueError("g2048: phase length must equal the number of boards")
    if out is None:
        out = torch.empty(boards.shape[0], dtype=torch.float64, device=boards.device)
    L.require_device_tensor(out, torch.float64, None, "out")
    L.call(boards.device, L.lib().g2048_eval, boards.data_ptr(), int(kind), phase.data_ptr() if phase is not None else None,
                               out.data_ptr(), boards.shape[0], L.stream_ptr(boards.device))
    return out


def obs(boards, out=None, dtype=torch.float32):
    """PPOAgent.normalize_state for every board (agents/ppo_agent.py:184-195): float32 (n,16); dtype=torch.float16 /
    torch.bfloat16 give the same values rounded once more (nearest even) for reduced-precision policies."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    if out is not None:
        dtype = out.dtype
    if dtype in (torch.float16, torch.bfloat16):
        if out is None:
            out = torch.empty((boards.shape[0], 16), dtype=dtype, device=boards.device)
        L.require_device_tensor(out, dtype, (16,), "out")
        L.call(boards.device, L.lib().g2048_obs_16, boards.data_ptr(), out.data_ptr(), int(dtype == torch.bfloat16),
               boards.shape[0], L.stream_ptr(boards.device))
        return out
    if out is None:
        out = torch.empty((boards.shape[0], 16), dtype=torch.float32, device=boards.device)
    L.require_device_tensor(out, torch.float32, (16,), "out")
    L.call(boards.device, L.lib().g2048_obs_f32, boards.data_ptr(), out.data_ptr(), boards.shape[0], L.stream_ptr(boards.device))
    return out


def track_episodes(flags, alive, moves, valid_cnt, invalid_cnt, milestone_move, move_index, expanded=None,
                   expanded_sum=None, keyblock=None):
    """One-kernel bookkeeping of the evaluation loop (reference evaluate_beam_search.py:42-64); all tensors are
    updated in place. alive uint8 (n,), moves/valid_cnt/invalid_cnt int32 (n,), milestone_move int32 (n,8)."""
    n = flags.shape[0]
    L.require_device_tensor(flags, torch.uint8, None, "flags")
    L.require_device_tensor(alive, torch.uint8, None, "alive")
    for name, t in (("moves", moves), ("valid_cnt", valid_cnt), ("invalid_cnt", invalid_cnt)):
        L.require_device_tensor(t, torch.int32, None, name)
    L.require_device_tensor(milestone_move, torch.int32, (8,), "milestone_move")
    if expanded is not None:
        L.require_device_tensor(expanded, torch.int32, None, "expanded")
        L.require_device_tensor(expanded_sum, torch.int64, None, "expanded_sum")
    args = (flags.data_ptr(), expanded.data_ptr() if expanded is not None else None, alive.data_ptr(), moves.data_ptr(),
            valid_cnt.data_ptr(), invalid_cnt.data_ptr(), milestone_move.data_ptr(),
            expanded_sum.data_ptr() if expanded is not None else None)
    if keyblock is not None:
        L.call(flags.device, L.lib().g2048_track_episodes_dyn, *args, keyblock.words.data_ptr(), n, L.stream_ptr(flags.device))
    else:
        L.call(flags.device, L.lib().g2048_track_episodes, *args, int(move_index), n, L.stream_ptr(flags.device))


def sample_actions(probs, mask4=None, seed=0x2048, step_index=0, id_base=0, actions=None, prob=None, keyblock=None):
    """Masked categorical sampling (PPOAgent.get_action, agents/ppo_agent.py:211-221) for every env in one kernel.
    probs float32 (n,4); mask4 uint8 (n,) or None. Returns (actions uint8 (n,), prob float32 (n,))."""
    L.require_device_tensor(probs, torch.float32, (4,), "probs")
    n = probs.shape[0]
    if mask4 is not None:
        L.require_device_tensor(mask4, torch.uint8, None, "mask4")
    dev = probs.device
    actions = _output(actions, n, torch.uint8, None, "actions", dev)
    prob = _output(prob, n, torch.float32, None, "prob", dev)
    mp = mask4.data_ptr() if mask4 is not None else None
    if keyblock is not None:
        L.call(dev, L.lib().g2048_sample_actions_dyn, probs.data_ptr(), mp, actions.data_ptr(), prob.data_ptr(),
               keyblock.words.data_ptr(), L.u64(id_base), n, L.stream_ptr(dev))
    else:
        L.call(dev, L.lib().g2048_sample_actions, probs.data_ptr(), mp, actions.data_ptr(), prob.data_ptr(), L.u64(seed),
               L.u64(step_index), L.u64(id_base), n, L.stream_ptr(dev))
    return actions, prob


_OBS_KIND = {torch.float32: L.OBS_F32, torch.float16: L.OBS_F16, torch.bfloat16: L.OBS_BF16}


def rollout_step(boards, probs, scores, seed, step_index, id_base=0, *, mask=None, out=None, actions=None, prob=None,
                 reward=None, flags=None, obs_next=None, mask_next=None, next_boards=None, state_maxcode=None,
                 auto_reset=True, step_counter=None):
    """One PPO rollout step of every env in ONE launch (include/g2048.h, g2048_rollout_step): masked sampling from
    `probs` (agents/ppo_agent.py:211-221) -> Game2048Env.step (environment/game_2048.py:170-210) -> next observation
    (ppo_agent.py:184-195, dtype of `obs_next`) and next valid-move mask (game_2048.py:69-95), all from registers.
    reward may be float32 or float64. step_counter: int64 device tensor added to step_index inside the kernel (for
    replayable hipGraphs). Returns (boards_out, actions, prob, reward, flags)."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    L.require_device_tensor(probs, torch.float32, (4,), "probs")
    _require_scores(scores)
    n, dev = boards.shape[0], boards.device
    if probs.shape[0] != n or scores.shape[0] != n:
        raise ValueError("g2048: probs/scores length must equal the number of boards")
    out = torch.empty_like(boards) if out is None else L.require_device_tensor(out, torch.uint8, (16,), "out")
    actions = torch.empty(n, dtype=torch.uint8, device=dev) if actions is None else L.require_device_tensor(actions, torch.uint8, None, "actions")
    prob = torch.empty(n, dtype=torch.float32, device=dev) if prob is None else L.require_device_tensor(prob, torch.float32, None, "prob")
    if reward is None:
        reward = torch.empty(n, dtype=torch.float32, device=dev)
    if reward.dtype not in (torch.float32, torch.float64):
        raise TypeError("g2048: reward must be float32 or float64")
    L.require_device_tensor(reward, reward.dtype, None, "reward")
    flags = torch.empty(n, dtype=torch.uint8, device=dev) if flags is None else L.require_device_tensor(flags, torch.uint8, None, "flags")
    opts = (L.STEP_REWARD_F64 if reward.dtype == torch.float64 else 0) | (L.STEP_AUTO_RESET if auto_reset else 0)
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    if mask is not None:
        L.require_device_tensor(mask, torch.uint8, None, "mask")
    if obs_next is not None:
        if obs_next.dtype not in _OBS_KIND:
            raise TypeError("g2048: obs_next must be float32, float16 or bfloat16")
        L.require_device_tensor(obs_next, obs_next.dtype, (16,), "obs_next")
        opts |= _OBS_KIND[obs_next.dtype] << L.ROLLOUT_OBS_SHIFT
    if mask_next is not None:
        L.require_device_tensor(mask_next, torch.uint8, None, "mask_next")
    if next_boards is not None:
        L.require_device_tensor(next_boards, torch.uint8, (16,), "next_boards")
    if state_maxcode is not None:
        L.require_device_tensor(state_maxcode, torch.uint8, None, "state_maxcode")
    if step_counter is not None:
        L.require_device_tensor(step_counter, torch.int64, None, "step_counter")
    for name, t in (("actions", actions), ("prob", prob), ("reward", reward), ("flags", flags), ("out", out), ("mask", mask),
                    ("obs_next", obs_next), ("mask_next", mask_next), ("next_boards", next_boards), ("state_maxcode", state_maxcode)):
        if t is not None and t.shape[0] != n:
            raise ValueError("g2048: %s must have one row per env" % name)
    L.call(dev, L.lib().g2048_rollout_step, boards.data_ptr(), probs.data_ptr(), ptr(mask), out.data_ptr(), scores.data_ptr(),
           actions.data_ptr(), prob.data_ptr(), reward.data_ptr(), flags.data_ptr(), ptr(obs_next), ptr(mask_next),
           ptr(next_boards), ptr(state_maxcode), L.u64(seed), L.u64(step_index), ptr(step_counter), L.u64(id_base), n, opts,
           L.stream_ptr(dev))
    return out, actions, prob, reward, flags


POLICY_PRECISIONS = {"f32": L.POLICY_F32, "bf16": L.POLICY_BF16}


def _pack(fn, plain, args, nb, out):
    """fn(plain, *args, out, stream) into `out`, a uint8 tensor of nb bytes (allocated when None)."""
    if out is None:
        out = torch.empty(nb, dtype=torch.uint8, device=plain.device)
    L.require_device_tensor(out, torch.uint8, None, "out")
    if out.numel() != nb:
        raise ValueError("g2048: out must hold %d bytes" % nb)
    L.call(plain.device, fn, plain.data_ptr(), *args, out.data_ptr(), L.stream_ptr(plain.device))
    return out


def policy_packed_bytes(precision="f32", n_out=4):
    """Bytes of one packed network (g2048_policy_packed_bytes)."""
    return _sized(L.lib().g2048_policy_packed_bytes(POLICY_PRECISIONS[precision], int(n_out)), "g2048: n_out must be 4 (actor) or 1 (critic)")


def policy_pack(plain, n_out, precision="f32", out=None):
    """Pack one network's plain float32 parameters (W1 b1 W2 b2 W3 b3 W4 b4 back to back, weights [out][in], BatchNorm folded
    in: include/g2048.h) into the blob g2048_policy_forward streams. Writes `out` (uint8, policy_packed_bytes) in place when
    given, on the current stream, without synchronising."""
    L.require_device_tensor(plain, torch.float32, None, "plain")
    if plain.dim() != 1 or plain.numel() != 45504 + 65 * int(n_out):
        raise ValueError("g2048: plain must be a flat float32 tensor of 45,504 + 65 * n_out parameters")
    return _pack(L.lib().g2048_policy_pack, plain, (int(n_out), POLICY_PRECISIONS[precision]), policy_packed_bytes(precision, n_out), out)


def policy_forward(boards, actor_packed, critic_packed=None, precision="f32", probs=None, value=None):
    """PPO actor (and critic) forward pass on the packed boards in ONE launch (g2048_policy_forward). Returns probs float32
    (n,4), or (probs, value float32 (n,1)) when critic_packed is given."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    n, dev = boards.shape[0], boards.device
    probs = _output(probs, n, torch.float32, (4,), "probs", dev)
    if critic_packed is not None or value is not None:
        value = _output(value, n, torch.float32, (1,), "value", dev)
    L.call(dev, L.lib().g2048_policy_forward, boards.data_ptr(), actor_packed.data_ptr(),
           critic_packed.data_ptr() if critic_packed is not None else None, probs.data_ptr(),
           value.data_ptr() if value is not None else None, n, POLICY_PRECISIONS[precision], L.stream_ptr(dev))
    return probs if critic_packed is None else (probs, value)


def tpolicy_plain_floats(dim_ff, n_layers):
    """Floats of the plain parameter buffer g2048_tpolicy_pack reads (include/g2048.h)."""
    return 128 + int(n_layers) * (16962 + 129 * int(dim_ff)) + 139781


def qnet_plain_floats(dim_ff, n_layers):
    """Floats of the plain parameter buffer g2048_qnet_pack reads (include/g2048.h)."""
    return 140132 + int(n_layers) * (66690 + 257 * int(dim_ff))


# what differs between the two encoder networks' blobs: the plain-float formula and the library's two symbols
_NETS = {"tpolicy": (tpolicy_plain_floats, "g2048_tpolicy_packed_bytes", "g2048_tpolicy_pack"),
         "qnet": (qnet_plain_floats, "g2048_qnet_packed_bytes", "g2048_qnet_pack")}


def _net_packed_bytes(kind, precision, dim_ff, n_layers):
    if precision not in POLICY_PRECISIONS:
        raise ValueError("g2048: precision must be 'f32' or 'bf16'")
    nb = getattr(L.lib(), _NETS[kind][1])(POLICY_PRECISIONS[precision], int(dim_ff), int(n_layers))
    if nb == 0:
        raise ValueError("g2048: dim_ff must be a multiple of 32 and n_layers at least 1")
    return nb


def _net_pack(kind, plain, dim_ff, n_layers, precision, out):
    L.require_device_tensor(plain, torch.float32, None, "plain")
    nb = _net_packed_bytes(kind, precision, dim_ff, n_layers)
    _flat_plain(plain, _NETS[kind][0](dim_ff, n_layers))
    return _pack(getattr(L.lib(), _NETS[kind][2]), plain, (int(dim_ff), int(n_layers), POLICY_PRECISIONS[precision]), nb, out)


def _check_blob(kind, packed, precision, dim_ff, n_layers):
    """A forward call's packed blob: a uint8 device tensor of the size of (precision, dim_ff, n_layers)."""
    L.require_device_tensor(packed, torch.uint8, None, "packed")
    nb = _net_packed_bytes(kind, precision, dim_ff, n_layers)
    if packed.numel() != nb:
        raise ValueError("g2048: packed must be a %s blob of %d bytes" % (precision, nb))


def tpolicy_packed_bytes(precision="f32", dim_ff=2048, n_layers=2):
    """Bytes of the packed transformer policy (g2048_tpolicy_packed_bytes)."""
    return _net_packed_bytes("tpolicy", precision, dim_ff, n_layers)


def tpolicy_pack(plain, dim_ff, n_layers, precision="f32", out=None):
    """Pack the transformer policy's plain float32 parameters (state-dict order plus the two LayerNorm eps per layer:
    include/g2048.h) into the blob g2048_tpolicy_forward streams. Writes `out` (uint8, tpolicy_packed_bytes) in place when
    given, on the current stream, without synchronising."""
    return _net_pack("tpolicy", plain, dim_ff, n_layers, precision, out)


def tpolicy_forward(boards, packed, dim_ff, n_layers, precision="f32", probs=None, value=None, want_value=True):
    """The transformer policy's forward pass on the packed boards in ONE launch (g2048_tpolicy_forward). Returns (probs
    float32 (n,4), value float32 (n,1)), or probs alone with want_value=False."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _check_blob("tpolicy", packed, precision, dim_ff, n_layers)
    n, dev = boards.shape[0], boards.device
    probs = _output(probs, n, torch.float32, (4,), "probs", dev)
    if want_value or value is not None:
        value = _output(value, n, torch.float32, (1,), "value", dev)
    L.call(dev, L.lib().g2048_tpolicy_forward, boards.data_ptr(), packed.data_ptr(), probs.data_ptr(),
           value.data_ptr() if value is not None else None, n, int(dim_ff), int(n_layers), POLICY_PRECISIONS[precision], L.stream_ptr(dev))
    return probs if value is None else (probs, value)


def tpolicy_grad_workspace_bytes(n, dim_ff, n_layers):
    """Bytes of the workspace tpolicy_loss_grad needs for n boards (g2048_tpolicy_grad_workspace, the learner library)."""
    return _sized(L.tlearn_lib().g2048_tpolicy_grad_workspace(int(n), int(dim_ff), int(n_layers)),
                  "g2048: tpolicy_loss_grad takes 1 .. %d boards (16 tokens each; a larger batch is refused, not truncated), a "
                  "dim_ff that is a multiple of 32 and 1 .. 64 layers (got n = %d, dim_ff = %d, n_layers = %d)",
                  L.TLEARN_BATCH_MAX, int(n), int(dim_ff), int(n_layers))


GRAD_PRECISIONS = ("f32", "bf16")


def check_grad_precision(grad_precision):
    if grad_precision not in GRAD_PRECISIONS:
        raise ValueError("g2048: grad_precision must be 'f32' or 'bf16' (got %r)" % (grad_precision,))
    return grad_precision


def tpolicy_bf16_workspace_bytes(n, dim_ff, n_layers):
    """Bytes of the workspace tpolicy_loss_grad with grad_precision="bf16" needs for n boards (g2048_tpolicy_bf16_workspace, the bf16
    learner library): tpolicy_train_workspace_bytes with the two (16 n, dim_ff) arrays at 2 bytes an element, plus 512 dim_ff bytes
    of packed weights a layer."""
    return _sized(L.tbf16_lib().g2048_tpolicy_bf16_workspace(int(n), int(dim_ff), int(n_layers)),
                  "g2048: the transformer policy's bf16 gradient pass takes 1 .. %d boards (16 tokens each; a larger batch is refused, "
                  "not truncated), a dim_ff that is a multiple of 32 and 1 .. 64 layers (got n = %d, dim_ff = %d, n_layers = %d)",
                  L.TLEARN_BATCH_MAX, int(n), int(dim_ff), int(n_layers))


def tpolicy_loss_grad(boards, plain, actions, old_log_probs, advantages, returns, dim_ff, n_layers, clip_epsilon=0.3, value_coef=0.4,
                      entropy_coef=0.05, grad=None, losses=None, probs=None, value=None, workspace=None, dropout=None, seed=0, call_index=0,
                      grad_precision="f32"):
    """PPOAgent.update()'s loss (agents/ppo_agent.py:378-400) on the transformer policy's two heads and its gradient, on the device
    (g2048_tpolicy_loss_grad, the learner library): probs, value = the eval-mode module on boards / 15; loss = actor + value_coef
    value_loss - entropy_coef entropy with the clipped surrogate of exp(log probs[i, actions[i]] - old_log_probs[i]) against
    advantages, the squared error of value against returns, and Categorical(probs)'s entropy; grad = d loss / d parameter in the
    layout of `plain` (the LayerNorm-eps slots 0), overwritten, never accumulated into. boards uint8 (n,16), actions int64 (n,),
    old_log_probs, advantages, returns float32 (n,), plain the PLAIN float32 parameter buffer (tpolicy_plain_floats). f32 only. An
    action outside 0..3 is the caller's error (the kernel reads actions & 3). A sequence of launches on the current stream, no
    synchronisation. dropout: None, 0 or all zeros: eval mode through the learner library, as ever. A probability or a 4-tuple
    (qnet_dropout_p): the module's TRAINING-mode pass with the masks of (seed, call_index) (tpolicy_dropout_mask), regenerated in
    the backward (the training library's g2048_tpolicy_loss_grad_dropout; the workspace is then tpolicy_train_workspace_bytes').
    grad_precision "bf16": the seven feed-forward products of every encoder layer take bf16 operands with f32 accumulation and the
    hidden layer and its gradient are kept as bf16 (g2048_tpolicy_loss_grad_bf16, the bf16 learner library, include/g2048_tbf16.h has
    the rounding points; the workspace is then tpolicy_bf16_workspace_bytes', with or without dropout). Not a rounding-level change:
    gradients move by per cents of their largest element. "f32", the default: the calls above, bit for bit.
    Returns (losses float32 (4,) = loss, actor, value, entropy; probs float32 (n,4); value float32 (n,1); grad)."""
    bf16 = check_grad_precision(grad_precision) == "bf16"
    p = qnet_dropout_p(dropout)
    floats = tpolicy_plain_floats(dim_ff, n_layers)
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _flat_plain(plain, floats)
    L.require_device_tensor(actions, torch.int64, (), "actions")
    for t, name in ((old_log_probs, "old_log_probs"), (advantages, "advantages"), (returns, "returns")):
        L.require_device_tensor(t, torch.float32, (), name)
    n, dev = boards.shape[0], boards.device
    if not (actions.shape[0] == old_log_probs.shape[0] == advantages.shape[0] == returns.shape[0] == n):
        raise ValueError("g2048: actions, old_log_probs, advantages and returns must have one entry per board")
    grad = _grad_output(grad, floats, dev)
    if losses is None:
        losses = torch.empty(4, dtype=torch.float32, device=dev)
    L.require_device_tensor(losses, torch.float32, None, "losses")
    if losses.numel() != 4:
        raise ValueError("g2048: losses must hold four float32")
    probs = _output(probs, n, torch.float32, (4,), "probs", dev)
    value = _output(value, n, torch.float32, (1,), "value", dev)
    if n == 0:
        return losses, probs, value, grad
    nb = (tpolicy_bf16_workspace_bytes if bf16 else tpolicy_grad_workspace_bytes if p is None else tpolicy_train_workspace_bytes)(
        n, dim_ff, n_layers)
    workspace = _workspace(workspace, nb, dev)
    if bf16:
        L.tbf16_call(dev, L.tbf16_lib().g2048_tpolicy_loss_grad_bf16, boards.data_ptr(), plain.data_ptr(), actions.data_ptr(),
                     old_log_probs.data_ptr(), advantages.data_ptr(), returns.data_ptr(), n, int(dim_ff), int(n_layers),
                     None if p is None else _p4(p), L.u64(seed), L.u64(call_index), float(clip_epsilon), float(value_coef), float(entropy_coef),
                     grad.data_ptr(), losses.data_ptr(), probs.data_ptr(), value.data_ptr(), workspace.data_ptr(), workspace.numel(),
                     L.stream_ptr(dev))
    elif p is None:
        L.tlearn_call(dev, L.tlearn_lib().g2048_tpolicy_loss_grad, boards.data_ptr(), plain.data_ptr(), actions.data_ptr(),
                      old_log_probs.data_ptr(), advantages.data_ptr(), returns.data_ptr(), n, int(dim_ff), int(n_layers), float(clip_epsilon),
                      float(value_coef), float(entropy_coef), grad.data_ptr(), losses.data_ptr(), probs.data_ptr(), value.data_ptr(),
                      workspace.data_ptr(), workspace.numel(), L.stream_ptr(dev))
    else:
        L.ttrain_call(dev, L.ttrain_lib().g2048_tpolicy_loss_grad_dropout, boards.data_ptr(), plain.data_ptr(), actions.data_ptr(),
                      old_log_probs.data_ptr(), advantages.data_ptr(), returns.data_ptr(), n, int(dim_ff), int(n_layers), _p4(p), L.u64(seed),
                      L.u64(call_index), float(clip_epsilon), float(value_coef), float(entropy_coef), grad.data_ptr(), losses.data_ptr(),
                      probs.data_ptr(), value.data_ptr(), workspace.data_ptr(), workspace.numel(), L.stream_ptr(dev))
    return losses, probs, value, grad


def tpolicy_train_workspace_bytes(n, dim_ff, n_layers):
    """Bytes of the workspace tpolicy_loss_grad with dropout and tpolicy_forward_train need for n boards
    (g2048_tpolicy_train_workspace, the training library): tpolicy_grad_workspace_bytes plus one (16 n, 64) float32 array."""
    return _sized(L.ttrain_lib().g2048_tpolicy_train_workspace(int(n), int(dim_ff), int(n_layers)),
                  "g2048: the transformer policy's training passes take 1 .. %d boards (16 tokens each; a larger batch is refused, "
                  "not truncated), a dim_ff that is a multiple of 32 and 1 .. 64 layers (got n = %d, dim_ff = %d, n_layers = %d)",
                  L.TLEARN_BATCH_MAX, int(n), int(dim_ff), int(n_layers))


def tpolicy_forward_train(boards, plain, dim_ff, n_layers, dropout, seed=0, call_index=0, probs=None, value=None, workspace=None):
    """The transformer policy's TRAINING-mode forward on uint8 (n,16) boards, in f32 from the PLAIN parameter buffer
    (g2048_tpolicy_forward_dropout, the training library): the forward launches of tpolicy_loss_grad with the masks of (seed,
    call_index) and the two heads; at equal (seed, call_index) the bits of the probs and value tpolicy_loss_grad returns. dropout:
    a probability or a 4-tuple (qnet_dropout_p; None, 0 or all zeros run the same launches without a mask). workspace: a uint8
    device tensor of at least tpolicy_train_workspace_bytes(n, dim_ff, n_layers) (allocated when None). No synchronisation.
    Returns (probs float32 (n,4), value float32 (n,1))."""
    p = qnet_dropout_p(dropout) or (0.0, 0.0, 0.0, 0.0)
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _flat_plain(plain, tpolicy_plain_floats(dim_ff, n_layers))
    n, dev = boards.shape[0], boards.device
    probs = _output(probs, n, torch.float32, (4,), "probs", dev)
    value = _output(value, n, torch.float32, (1,), "value", dev)
    if n == 0:
        return probs, value
    workspace = _workspace(workspace, tpolicy_train_workspace_bytes(n, dim_ff, n_layers), dev)
    L.ttrain_call(dev, L.ttrain_lib().g2048_tpolicy_forward_dropout, boards.data_ptr(), plain.data_ptr(), n, int(dim_ff), int(n_layers), _p4(p),
                  L.u64(seed), L.u64(call_index), probs.data_ptr(), value.data_ptr(), workspace.data_ptr(), workspace.numel(), L.stream_ptr(dev))
    return probs, value


def tpolicy_dropout_mask(n, layer, site, p, dim_ff=2048, seed=0, call_index=0, first_row=0, rows=None, device="cuda", out=None):
    """The keep bits of rows [first_row, first_row + rows) of one dropout site of one call of the transformer policy's training
    passes (g2048_tpolicy_dropout_mask), written through the function the kernels draw them with: uint8 (rows, columns), 1 where
    the element is kept. The site's matrix is (64 n, 16) for site 0 (row = (board 4 + head) 16 + query, column = key), (16 n, 64)
    for sites 1 and 3 and (16 n, dim_ff) for site 2 (row = token = 16 board + cell); rows None: down to the matrix's last row.
    Element e = row columns + column of site s of encoder layer `layer` is kept iff rng_draw(rng_keys(seed, 13, call_index),
    ((4 layer + s) << 32) | e, 0) >= floor(p 2^32); a kept element is multiplied by float32(1 / (1 - p)), a dropped one by 0. No
    synchronisation."""
    return _encoder_dropout_mask("tpolicy", n, layer, site, p, dim_ff, seed, call_index, first_row, rows, device, out)


def tpolicy_step_workspace_bytes(dim_ff, n_layers):
    """Bytes of the workspace tpolicy_adam_step needs (g2048_tpolicy_step_workspace, the step library): one float64 per partial sum
    of the norm and the scalars its second launch prepares."""
    return _sized(L.tstep_lib().g2048_tpolicy_step_workspace(int(dim_ff), int(n_layers)),
                  "g2048: tpolicy_adam_step takes a dim_ff that is a multiple of 32 and 1 .. 64 layers (got dim_ff = %d, "
                  "n_layers = %d)",
                  int(dim_ff), int(n_layers))


def tpolicy_adam_step(plain, grad, exp_avg, exp_avg_sq, dim_ff, n_layers, counters, losses=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-8,
                      max_norm=0.5, norm=None, workspace=None):
    """What follows backward() in an epoch of PPOAgent.update (agents/ppo_agent.py:403-416) for the transformer policy in three
    launches (g2048_tpolicy_adam_step, the step library): the NaN check on losses[0], clip_grad_norm_(max_norm) and an Adam step.
    plain, grad, exp_avg and exp_avg_sq are flat float32 device tensors of tpolicy_plain_floats(dim_ff, n_layers) in the plain
    layout, all updated IN PLACE (grad is left clipped); counters is int64 (3,) on the device = {steps applied, calls skipped for a
    NaN loss, calls skipped for a gradient norm that is not finite}, and the bias correction's step number is taken from it ON THE
    DEVICE. losses: tpolicy_loss_grad's float32 (4,) (or any float32 tensor whose first element is the loss), None: no loss gate.
    max_norm None means no clipping. The LayerNorm-eps slots keep their bits in all four buffers. A NaN loss or a norm that is not
    finite leaves all four buffers and the step counter untouched. No synchronisation. Returns the gradient norm before clipping,
    float32, written on every call."""
    floats = tpolicy_plain_floats(dim_ff, n_layers)
    dev = _step_buffers((("plain", plain, floats), ("grad", grad, floats), ("exp_avg", exp_avg, floats), ("exp_avg_sq", exp_avg_sq, floats)))
    _step_counters(counters, 3)
    _gate_losses(losses)
    norm = _float_output(norm, (), "norm", dev)
    workspace = _workspace(workspace, tpolicy_step_workspace_bytes(dim_ff, n_layers), dev)
    for t, name in ((counters, "counters"), (losses, "losses"), (norm, "norm"), (workspace, "workspace")):
        if t is not None and t.device != dev:
            raise ValueError("g2048: %s on %s, plain on %s" % (name, t.device, dev))
    L.tstep_call(dev, L.tstep_lib().g2048_tpolicy_adam_step, plain.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                 int(dim_ff), int(n_layers), losses.data_ptr() if losses is not None else None, counters.data_ptr(), float(lr),
                 float(betas[0]), float(betas[1]), float(eps), float("inf") if max_norm is None else float(max_norm), norm.data_ptr(),
                 workspace.data_ptr(), workspace.numel(), L.stream_ptr(dev))
    return norm


def qnet_packed_bytes(precision="f32", dim_ff=2048, n_layers=2):
    """Bytes of the packed hybrid Q-network (g2048_qnet_packed_bytes)."""
    return _net_packed_bytes("qnet", precision, dim_ff, n_layers)


def qnet_pack(plain, dim_ff, n_layers, precision="f32", out=None):
    """Pack the hybrid Q-network's plain float32 parameters (state-dict order plus the two LayerNorm eps per layer:
    include/g2048.h) into the blob g2048_qnet_forward streams. Writes `out` (uint8, qnet_packed_bytes) in place when given, on
    the current stream, without synchronising."""
    return _net_pack("qnet", plain, dim_ff, n_layers, precision, out)


def qnet_forward(boards, packed, dim_ff, n_layers, precision="f32", q=None, actions=None, want_actions=False):
    """The hybrid agent's Q-network on the packed boards in ONE launch (g2048_qnet_forward). Returns q float32 (n,4), or (actions
    uint8 (n,), q) when `actions` is given or want_actions is set: the exploit action of DQNAgent.select_action (the argmax of q
    over the env's valid moves, ties to the lowest index, 0 for a board with no valid move)."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _check_blob("qnet", packed, precision, dim_ff, n_layers)
    n, dev = boards.shape[0], boards.device
    q = _output(q, n, torch.float32, (4,), "q", dev)
    if want_actions or actions is not None:
        actions = _output(actions, n, torch.uint8, (), "actions", dev)
    L.call(dev, L.lib().g2048_qnet_forward, boards.data_ptr(), packed.data_ptr(), q.data_ptr(),
           actions.data_ptr() if actions is not None else None, n, int(dim_ff), int(n_layers), POLICY_PRECISIONS[precision],
           L.stream_ptr(dev))
    return q if actions is None else (actions, q)


def qnet_batch_workspace_bytes(n, dim_ff):
    """Bytes of the workspace qnet_forward_batch needs for n boards (g2048_qnet_batch_workspace)."""
    return _sized(L.lib().g2048_qnet_batch_workspace(int(n), int(dim_ff)),
                  "g2048: qnet_forward_batch takes 1 .. %d boards (they are one sequence; a larger batch is refused, not "
                  "truncated) and a dim_ff that is a multiple of 32 (got n = %d, dim_ff = %d)",
                  L.QNET_BATCH_MAX, int(n), int(dim_ff))


QNET_DROPOUT_SITES = ("attention", "dropout1", "dropout", "dropout2")       # the order torch's training-mode layer draws in


def qnet_dropout_p(dropout, name="dropout"):
    """The four dropout probabilities of an encoder layer as the training library takes them, in the order of
    QNET_DROPOUT_SITES: None or one probability for all four sites, or a 4-tuple; each finite, 0 <= p < 1. Returns None when
    every site is off (the passes are then the main library's, bit for bit)."""
    if dropout is None:
        return None
    if isinstance(dropout, (tuple, list)):
        if len(dropout) != 4:
            raise ValueError("g2048: %s must be a probability or a 4-tuple %s" % (name, QNET_DROPOUT_SITES))
        p = tuple(float(v) for v in dropout)
    else:
        p = (float(dropout),) * 4
    for v in p:
        if not 0.0 <= v < 1.0:              # a NaN fails both comparisons
            raise ValueError("g2048: %s must be finite, 0 <= p < 1 (got %r)" % (name, v))
    return p if any(p) else None


# what differs between the two encoder networks' dropout masks: the batch limit, what the message calls it, the site's matrix
# (rows, columns) of n boards, and the library and entry point that write it
_MASKS = {"qnet": (L.QNET_BATCH_MAX, "the batch passes' limit", lambda site, n, dim_ff: (8 * n, n) if site == 0 else (n, dim_ff if site == 2 else 128),
                   L.TRAIN, "g2048_qnet_dropout_mask"),
          "tpolicy": (L.TLEARN_BATCH_MAX, "the gradient pass's limit",
                      lambda site, n, dim_ff: (64 * n, 16) if site == 0 else (16 * n, dim_ff if site == 2 else 64),
                      L.TTRAIN, "g2048_tpolicy_dropout_mask")}


def _encoder_dropout_mask(kind, n, layer, site, p, dim_ff, seed, call_index, first_row, rows, device, out):
    limit, limit_name, site_shape, library, entry = _MASKS[kind]
    n, layer, site, first_row = int(n), int(layer), int(site), int(first_row)
    if site not in (0, 1, 2, 3):
        raise ValueError("g2048: site must be 0 .. 3 %s" % (QNET_DROPOUT_SITES,))
    if not 0 <= layer < 64:
        raise ValueError("g2048: layer must be 0 .. 63")
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("g2048: p must be finite, 0 <= p < 1 (got %r)" % p)
    if not 0 <= n <= limit:
        raise ValueError("g2048: a dropout mask is of 0 .. %d boards (%s); got n = %d" % (limit, limit_name, n))
    height, width = site_shape(site, n, int(dim_ff))
    rows = height - first_row if rows is None else int(rows)
    if first_row < 0 or rows < 0 or first_row + rows > height:
        raise ValueError("g2048: rows %d .. %d lie past the site's matrix of %d rows" % (first_row, first_row + rows, height))
    dev = torch.device(device)
    out = _output(out, rows, torch.uint8, (width,), "out", dev)
    if n and rows:
        library.call(out.device, getattr(library.load(), entry), L.u64(seed), L.u64(call_index), layer, site, p, n, int(dim_ff), first_row, rows,
                     out.data_ptr(), L.stream_ptr(out.device))
    return out


def _p4(p):
    return (C.c_double * 4)(*p)


def qnet_dropout_mask(n, layer, site, p, dim_ff=2048, seed=0, call_index=0, first_row=0, rows=None, device="cuda", out=None):
    """The keep bits of rows [first_row, first_row + rows) of one dropout site of one call (g2048_qnet_dropout_mask), written
    through the function the training passes draw them with: uint8 (rows, columns), 1 where the element is kept. The site's
    matrix is (8 n, n) for site 0 (row = head n + query, column = key), (n, 128) for sites 1 and 3 and (n, dim_ff) for site 2;
    rows None: down to the matrix's last row. Element e = row columns + column of site s of encoder layer `layer` is kept iff
    rng_draw(rng_keys(seed, 12, call_index), ((4 layer + s) << 32) | e, 0) >= floor(p 2^32); a kept element is multiplied by
    float32(1 / (1 - p)), a dropped one by 0. No synchronisation."""
    return _encoder_dropout_mask("qnet", n, layer, site, p, dim_ff, seed, call_index, first_row, rows, device, out)


def qnet_train_workspace_bytes(n, dim_ff, n_layers):
    """Bytes of the workspace qnet_loss_grad needs for n boards with dropout (g2048_qnet_train_workspace)."""
    return _sized(L.train_lib().g2048_qnet_train_workspace(int(n), int(dim_ff), int(n_layers)),
                  "g2048: qnet_loss_grad takes 1 .. %d boards (they are one sequence; a larger batch is refused, not "
                  "truncated), a dim_ff that is a multiple of 32 and 1 .. 64 layers (got n = %d, dim_ff = %d, n_layers = %d)",
                  L.QNET_BATCH_MAX, int(n), int(dim_ff), int(n_layers))


def qnet_forward_batch(boards, plain, dim_ff, n_layers, q=None, workspace=None, dropout=None, seed=0, call_index=0):
    """The hybrid agent's Q-network on n boards as ONE call of the reference's module (g2048_qnet_forward_batch): the boards are
    one sequence of n tokens that attend to each other, as in DQNAgent.train_step. plain: the PLAIN float32 parameter buffer
    (qnet_plain_floats; qnet.flatten), read directly; f32 only. 2 + 5 n_layers launches on the current stream, no
    synchronisation. workspace: a uint8 device tensor of at least qnet_batch_workspace_bytes(n, dim_ff) (allocated when None).
    dropout: None, 0 or all zeros: the eval-mode function through the main library, as ever. A probability or a 4-tuple
    (qnet_dropout_p): the module's TRAINING-mode call with the masks of (seed, call_index) (qnet_dropout_mask), through the
    training library's g2048_qnet_forward_batch_dropout; same launches, same workspace. Returns q float32 (n,4)."""
    p = qnet_dropout_p(dropout)
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _flat_plain(plain, qnet_plain_floats(dim_ff, n_layers))
    n, dev = boards.shape[0], boards.device
    q = _output(q, n, torch.float32, (4,), "q", dev)
    if n == 0:
        return q
    workspace = _workspace(workspace, qnet_batch_workspace_bytes(n, dim_ff), dev)
    if p is None:
        L.call(dev, L.lib().g2048_qnet_forward_batch, boards.data_ptr(), plain.data_ptr(), q.data_ptr(), n, int(dim_ff), int(n_layers),
               workspace.data_ptr(), L.stream_ptr(dev))
    else:
        L.train_call(dev, L.train_lib().g2048_qnet_forward_batch_dropout, boards.data_ptr(), plain.data_ptr(), q.data_ptr(), n, int(dim_ff),
                     int(n_layers), _p4(p), L.u64(seed), L.u64(call_index), workspace.data_ptr(), L.stream_ptr(dev))
    return q


def qnet_grad_workspace_bytes(n, dim_ff, n_layers):
    """Bytes of the workspace qnet_loss_grad needs for n boards (g2048_qnet_grad_workspace)."""
    return _sized(L.lib().g2048_qnet_grad_workspace(int(n), int(dim_ff), int(n_layers)),
                  "g2048: qnet_loss_grad takes 1 .. %d boards (they are one sequence; a larger batch is refused, not "
                  "truncated), a dim_ff that is a multiple of 32 and 1 .. 64 layers (got n = %d, dim_ff = %d, n_layers = %d)",
                  L.QNET_BATCH_MAX, int(n), int(dim_ff), int(n_layers))


def qnet_loss_grad(boards, plain, actions, targets, weights, dim_ff, n_layers, grad=None, td=None, loss=None, q=None, workspace=None,
                   dropout=None, seed=0, call_index=0):
    """The gradient half of DQNAgent.train_step (agents/hybrid.py:1038, :1049-1055) on the device (g2048_qnet_loss_grad): q =
    the batch forward of qnet_forward_batch (the same bits), td = the Huber error of q[i, actions[i]] against targets[i], loss =
    mean(weights * td) and grad = d loss / d parameter in the layout of `plain` (the LayerNorm-eps slots 0), overwritten, never
    accumulated into. boards uint8 (n,16), actions int64 (n,), targets and weights float32 (n,), plain the PLAIN float32
    parameter buffer. f32 only. An action outside 0..3 is the caller's error (the kernel reads actions & 3). dropout: None, 0
    or all zeros: eval mode through the main library, as ever. A probability or a 4-tuple (qnet_dropout_p): the reference's
    TRAINING-mode pass with the masks of (seed, call_index), regenerated in the backward (the training library's
    g2048_qnet_loss_grad_dropout; the workspace is then qnet_train_workspace_bytes'). No synchronisation. Returns (loss float32 (),
    td float32 (n,), q float32 (n,4), grad float32 (plain.numel(),))."""
    p = qnet_dropout_p(dropout)
    floats = qnet_plain_floats(dim_ff, n_layers)
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _flat_plain(plain, floats)
    L.require_device_tensor(actions, torch.int64, (), "actions")
    L.require_device_tensor(targets, torch.float32, (), "targets")
    L.require_device_tensor(weights, torch.float32, (), "weights")
    n, dev = boards.shape[0], boards.device
    if not (actions.shape[0] == targets.shape[0] == weights.shape[0] == n):
        raise ValueError("g2048: actions, targets and weights must have one entry per board")
    grad = _grad_output(grad, floats, dev)
    td = _output(td, n, torch.float32, (), "td", dev)
    q = _output(q, n, torch.float32, (4,), "q", dev)
    loss = _float_output(loss, (), "loss", dev)
    if n == 0:
        return loss, td, q, grad
    nb = qnet_grad_workspace_bytes(n, dim_ff, n_layers) if p is None else qnet_train_workspace_bytes(n, dim_ff, n_layers)
    workspace = _workspace(workspace, nb, dev)
    if p is None:
        L.call(dev, L.lib().g2048_qnet_loss_grad, boards.data_ptr(), plain.data_ptr(), actions.data_ptr(), targets.data_ptr(),
               weights.data_ptr(), n, int(dim_ff), int(n_layers), grad.data_ptr(), td.data_ptr(), loss.data_ptr(), q.data_ptr(),
               workspace.data_ptr(), L.stream_ptr(dev))
    else:
        L.train_call(dev, L.train_lib().g2048_qnet_loss_grad_dropout, boards.data_ptr(), plain.data_ptr(), actions.data_ptr(),
                     targets.data_ptr(), weights.data_ptr(), n, int(dim_ff), int(n_layers), _p4(p), L.u64(seed), L.u64(call_index),
                     grad.data_ptr(), td.data_ptr(), loss.data_ptr(), q.data_ptr(), workspace.data_ptr(), L.stream_ptr(dev))
    return loss, td, q, grad


def qnet_step_workspace_bytes(dim_ff, n_layers):
    """Bytes of the workspace qnet_adamw_step needs (g2048_qnet_step_workspace): one float64 per partial sum of the norm."""
    return _sized(L.lib().g2048_qnet_step_workspace(int(dim_ff), int(n_layers)),
                  "g2048: qnet_adamw_step takes a dim_ff that is a multiple of 32 and 1 .. 64 layers (got dim_ff = %d, "
                  "n_layers = %d)",
                  int(dim_ff), int(n_layers))


def qnet_adamw_step(plain, grad, exp_avg, exp_avg_sq, dim_ff, n_layers, lr, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4,
                    max_norm=10.0, norm=None, workspace=None):
    """clip_grad_norm_(max_norm) and AdamW.step() of DQNAgent.train_step (agents/hybrid.py:1057-1058) over the whole Q-network in
    two launches (g2048_qnet_adamw_step): plain, grad, exp_avg and exp_avg_sq are flat float32 device tensors of
    qnet_plain_floats(dim_ff, n_layers) in the plain layout, all updated IN PLACE (grad is left clipped); step >= 1 is the number
    of this update; max_norm None means no clipping. The LayerNorm-eps slots keep their bits in all four. A gradient norm that
    is not finite leaves all four untouched. No synchronisation. Returns the gradient norm before clipping, float32 ()."""
    floats = qnet_plain_floats(dim_ff, n_layers)
    dev = _step_buffers((("plain", plain, floats), ("grad", grad, floats), ("exp_avg", exp_avg, floats), ("exp_avg_sq", exp_avg_sq, floats)))
    norm = _float_output(norm, (), "norm", dev)
    workspace = _workspace(workspace, qnet_step_workspace_bytes(dim_ff, n_layers), dev)
    L.call(dev, L.lib().g2048_qnet_adamw_step, plain.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
           int(dim_ff), int(n_layers), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
           float("inf") if max_norm is None else float(max_norm), int(step), norm.data_ptr(), workspace.data_ptr(), L.stream_ptr(dev))
    return norm


def dqn_targets(q_online_next, q_target_next, shaped, dones, gamma=0.99, targets=None, next_actions=None):
    """The Double-DQN targets of DQNAgent.train_step (agents/hybrid.py:1042-1046) in ONE launch (g2048_dqn_targets), given the
    online and the target network's Q float32 (n,4) on the next states, shaped and dones float32 (n,): next_actions int64 (n,) =
    the unmasked argmax of q_online_next (first maximum), targets float32 (n,) = shaped + (1 - dones) * gamma * q_target_next at
    that action, in torch's order of operations, bit for bit. Returns (targets, next_actions)."""
    L.require_device_tensor(q_online_next, torch.float32, (4,), "q_online_next")
    L.require_device_tensor(q_target_next, torch.float32, (4,), "q_target_next")
    L.require_device_tensor(shaped, torch.float32, (), "shaped")
    L.require_device_tensor(dones, torch.float32, (), "dones")
    n, dev = q_online_next.shape[0], q_online_next.device
    if not (q_target_next.shape[0] == shaped.shape[0] == dones.shape[0] == n):
        raise ValueError("g2048: the two Q, shaped and dones must have one row per transition")
    targets = _output(targets, n, torch.float32, (), "targets", dev)
    next_actions = _output(next_actions, n, torch.int64, (), "next_actions", dev)
    L.call(dev, L.lib().g2048_dqn_targets, q_online_next.data_ptr(), q_target_next.data_ptr(), shaped.data_ptr(), dones.data_ptr(),
           float(gamma), next_actions.data_ptr(), targets.data_ptr(), n, L.stream_ptr(dev))
    return targets, next_actions


def qnet_select_actions(q, boards, epsilon, seed=0x2048, step_index=0, id_base=0, actions=None, explored=None):
    """DQNAgent.select_action (hybrid.py:909-953, use_beam_search = False) for every board in ONE launch
    (g2048_qnet_select_actions), given q float32 (n,4) of qnet_forward: with probability epsilon (the coin is draw 1 of (seed,
    POLICY, step_index, id_base + i)) the reference's biased exploration among the valid moves (draw 0), otherwise the exploit
    action of qnet_forward. Returns (actions uint8 (n,), explored uint8 (n,): 1 where the board explored)."""
    epsilon = float(epsilon)
    if not 0.0 <= epsilon <= 1.0:
        raise ValueError("g2048: epsilon must lie in [0, 1]")
    L.require_device_tensor(q, torch.float32, (4,), "q")
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    n, dev = boards.shape[0], boards.device
    if q.shape[0] != n:
        raise ValueError("g2048: q must have n rows")
    actions = _output(actions, n, torch.uint8, (), "actions", dev)
    explored = _output(explored, n, torch.uint8, (), "explored", dev)
    L.call(dev, L.lib().g2048_qnet_select_actions, q.data_ptr(), boards.data_ptr(), actions.data_ptr(), explored.data_ptr(), epsilon,
           L.u64(seed), L.u64(step_index), L.u64(id_base), n, L.stream_ptr(dev))
    return actions, explored


def _check_beam_settings(beam_width, search_depth, threshold):
    if not 1 <= int(beam_width) <= 64:
        raise ValueError("g2048: beam_width must lie in 1 .. 64")
    if int(search_depth) < 1:
        raise ValueError("g2048: search_depth must be at least 1")
    if int(threshold) < 1:
        raise ValueError("g2048: threshold (beam_search_threshold, a tile value) must be at least 1")


def qnet_beam_actions(q, boards, succ_q=None, beam_width=15, search_depth=30, threshold=64, gamma=0.99, epsilon=0.0, seed=0x2048,
                      step_index=0, id_base=0, actions=None, planned=None, explored=None):
    """DQNAgent.select_action with use_beam_search = True (hybrid.py:909-953) for every board in ONE launch
    (g2048_qnet_beam_actions), given q float32 (n,4) of qnet_forward: qnet_select_actions (same coin, same exploration, same
    draws) whose exploit action is the reference's beam_search where it plans -- max tile >= threshold and at least 8 tiles --
    and the argmax of q elsewhere. The search is one ranking of the board's at most 24 children (include/g2048.h); at
    search_depth >= 2 it consults no network, at search_depth 1 it reads succ_q float32 (n,32,4): qnet_forward of
    qnet_beam_expand's boards. Returns (actions uint8 (n,), planned uint8 (n,): 1 where the board is planned, explored uint8
    (n,))."""
    epsilon, gamma = float(epsilon), float(gamma)
    if not 0.0 <= epsilon <= 1.0:
        raise ValueError("g2048: epsilon must lie in [0, 1]")
    _check_beam_settings(beam_width, search_depth, threshold)
    if gamma != gamma or gamma in (float("inf"), -float("inf")):
        raise ValueError("g2048: gamma must be finite")
    if int(search_depth) == 1 and succ_q is None:
        raise ValueError("g2048: search_depth 1 needs succ_q, the Q-values of qnet_beam_expand's boards")
    L.require_device_tensor(q, torch.float32, (4,), "q")
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    n, dev = boards.shape[0], boards.device
    if q.shape[0] != n:
        raise ValueError("g2048: q must have n rows")
    if succ_q is not None:
        L.require_device_tensor(succ_q, torch.float32, (32, 4), "succ_q")
        if succ_q.shape[0] != n:
            raise ValueError("g2048: succ_q must have n rows")
    actions = _output(actions, n, torch.uint8, (), "actions", dev)
    planned = _output(planned, n, torch.uint8, (), "planned", dev)
    explored = _output(explored, n, torch.uint8, (), "explored", dev)
    L.call(dev, L.lib().g2048_qnet_beam_actions, q.data_ptr(), boards.data_ptr(), succ_q.data_ptr() if succ_q is not None else None,
           actions.data_ptr(), planned.data_ptr(), explored.data_ptr(), int(beam_width), int(search_depth), int(threshold), gamma,
           epsilon, L.u64(seed), L.u64(step_index), L.u64(id_base), n, L.stream_ptr(dev))
    return actions, planned, explored


def qnet_beam_expand(boards, seed=0x2048, step_index=0, id_base=0, succ=None, count=None):
    """The candidate boards of the reference's beam_search for every board in ONE launch (g2048_qnet_beam_expand): succ uint8
    (n,32,16), slot 8 a + j = candidate j of action a (the hybrid agent's simulate_move: up to three sampled empty cells x {2, 4};
    pick i of action a from draw 3 a + i of (seed, SIMULATE, step_index, id_base + row)); count uint8 (n,4). An invalid move has
    count 1 and the board itself in slot 8 a; unused slots are the empty board. Returns (succ, count)."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    n, dev = boards.shape[0], boards.device
    succ = _output(succ, n, torch.uint8, (32, 16), "succ", dev)
    count = _output(count, n, torch.uint8, (4,), "count", dev)
    L.call(dev, L.lib().g2048_qnet_beam_expand, boards.data_ptr(), succ.data_ptr(), count.data_ptr(), L.u64(seed), L.u64(step_index),
           L.u64(id_base), n, L.stream_ptr(dev))
    return succ, count


class SeenStates:
    """The `seen_states` set and `highest_tile_seen` of PPOAgent (agents/ppo_agent.py:171-176) for ordered batches of
    transitions, resident on the GPU: an open-addressing hash set keyed by the 16-byte board (include/g2048.h,
    g2048_seen_insert) that grows by rehashing, the running highest log2 code, and the running transition index."""

    def __init__(self, device="cuda", capacity_log2=20):
        self.device = torch.device(device)
        self.capacity_log2 = int(capacity_log2)
        self.table = torch.zeros((1 << self.capacity_log2, L.SEEN_SLOT_BYTES), dtype=torch.uint8, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.highest = torch.ones(1, dtype=torch.int32, device=self.device)     # log2 code of tile 2 (ppo_agent.py:171)
        self.index = 0              # transitions presented so far (global order)
        self._count_bound = 0       # host-side upper bound of the number of keys in the table (see reserve)

    def reserve(self, n_new):
        """Make room for n_new more transitions without overflowing: the table is kept at most half full of the keys it
        COULD hold. The host tracks an upper bound of the key count (the last count read back + every transition presented
        since); only when that bound no longer fits does it read the true count back (the one host sync, also the point where
        the overflow flag is looked at) and, if needed, grow by rehashing into a zeroed table with twice the room required --
        so in the steady state of a long run (many more keys than transitions per batch) batches are enqueued without any
        host round trip."""
        n_new = int(n_new)
        if 2 * (self._count_bound + n_new) <= (1 << self.capacity_log2):
            self._count_bound += n_new
            return
        self.assert_ok()                                    # host sync: overflow flag ...
        count = int(self.count.item())                      # ... and the true key count
        need = count + n_new
        if 2 * (need + n_new) > (1 << self.capacity_log2):      # (room for one more batch like this one under the bound, too)
            log2 = self.capacity_log2
            while (1 << log2) < 4 * need:                   # twice the room needed now: the next batches fit under the bound
                log2 += 1
            if log2 > 31:
                raise RuntimeError("g2048: seen-states table would exceed 2^31 slots")
            new = torch.zeros((1 << log2, L.SEEN_SLOT_BYTES), dtype=torch.uint8, device=self.device)
            L.call(self.device, L.lib().g2048_seen_rehash, self.table.data_ptr(), self.capacity_log2, new.data_ptr(), log2,
                   self.overflow.data_ptr(), L.stream_ptr(self.device))
            self.table, self.capacity_log2 = new, log2
        self._count_bound = need

    def assert_ok(self):
        """Raise if an insert ever found the table full or gave up probing (host sync). reserve() makes that impossible for
        batches that go through remember_shaping; call this after the LAST batch of a run, or pass check=True there."""
        flag = int(self.overflow.item())
        if flag:
            raise RuntimeError("g2048: the seen-states table overflowed (flag 0x%x): novelty terms of the batches since the last "
                               "check are not trustworthy -- it is sized by reserve(); was it bypassed?" % flag)

    def __len__(self):
        return int(self.count.item())


def remember_shaping(seen, next_boards, state_maxcode, flags, env_reward, out=None, want_novel=False, check=False):
    """PPOAgent.remember's stored reward (agents/ppo_agent.py:234-269) for an ORDERED batch of transitions, with the
    reference's sequential semantics for both stateful terms, continuing from `seen` (a SeenStates). Inputs are flat in
    order: next_boards uint8 (n,16) -- the next state BEFORE any auto-reset --, state_maxcode uint8 (n,), flags uint8 (n,)
    as the step wrote them, env_reward float64 (n,). Returns shaped float64 (n,) [, novel uint8 (n,)]. check=True reads the
    table's overflow flag back after THIS batch (one host sync) and raises if it is set; without it the flag is looked at
    the next time the table has to be re-sized, or by seen.assert_ok()."""
    L.require_device_tensor(next_boards, torch.uint8, (16,), "next_boards")
    n, dev = next_boards.shape[0], next_boards.device
    L.require_device_tensor(state_maxcode, torch.uint8, None, "state_maxcode")
    L.require_device_tensor(flags, torch.uint8, None, "flags")
    L.require_device_tensor(env_reward, torch.float64, None, "env_reward")
    if not (state_maxcode.shape[0] == flags.shape[0] == env_reward.shape[0] == n):
        raise ValueError("g2048: all transition arrays must have the same length")
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=dev)
    L.require_device_tensor(out, torch.float64, None, "out")
    if n == 0:
        return (out, torch.empty(0, dtype=torch.uint8, device=dev)) if want_novel else out

    def aligned(t, a):      # slices of larger tensors are contiguous but may start anywhere; the kernels use 16-byte loads
        return t if t.data_ptr() % a == 0 else t.clone()
    next_boards, flags, env_reward = aligned(next_boards, 16), aligned(flags, 16), aligned(env_reward, 8)
    seen.reserve(n)
    lib, st = L.lib(), L.stream_ptr(dev)
    ws = torch.empty(int(lib.g2048_shaping_scan_workspace(n)), dtype=torch.uint8, device=dev)
    prev_highest = torch.empty(n, dtype=torch.uint8, device=dev)
    slots = torch.empty(n, dtype=torch.int32, device=dev)
    novel = torch.empty(n, dtype=torch.uint8, device=dev) if want_novel else None
    L.call(dev, lib.g2048_shaping_scan, flags.data_ptr(), prev_highest.data_ptr(), seen.highest.data_ptr(), ws.data_ptr(), n, st)
    L.call(dev, lib.g2048_seen_insert, next_boards.data_ptr(), L.u64(seen.index), seen.table.data_ptr(), seen.capacity_log2,
           seen.count.data_ptr(), seen.overflow.data_ptr(), slots.data_ptr(), n, st)
    L.call(dev, lib.g2048_shaping_apply, next_boards.data_ptr(), state_maxcode.data_ptr(), flags.data_ptr(), env_reward.data_ptr(),
           prev_highest.data_ptr(), seen.table.data_ptr(), slots.data_ptr(), L.u64(seen.index), out.data_ptr(),
           novel.data_ptr() if novel is not None else None, n, st)
    seen.index += n
    if check:
        seen.assert_ok()
    return (out, novel) if want_novel else out


def simulate_move(boards, actions, highest_code=None):
    """Game2048Env.simulate_move for every (board, action) (environment/game_2048.py:341-387).
    Returns (succ uint8 (n,32,16), reward float64 (n,32), done bool (n,32), count uint8 (n,)); only the first
    count[i] slots of row i are successors, in the reference's order."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    L.require_device_tensor(actions, torch.uint8, None, "actions")
    n = boards.shape[0]
    if actions.shape[0] != n:
        raise ValueError("g2048: actions length must equal the number of boards")
    if highest_code is not None:
        L.require_device_tensor(highest_code, torch.uint8, None, "highest_code")
    dev = boards.device
    succ = torch.empty((n, 32, 16), dtype=torch.uint8, device=dev)
    reward = torch.empty((n, 32), dtype=torch.float64, device=dev)
    done = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    count = torch.empty(n, dtype=torch.uint8, device=dev)
    L.call(dev, L.lib().g2048_simulate_move, boards.data_ptr(), actions.data_ptr(),
                                        highest_code.data_ptr() if highest_code is not None else None,
                                        succ.data_ptr(), reward.data_ptr(), done.data_ptr(), count.data_ptr(), n,
                                        L.stream_ptr(dev))
    return succ, reward, done.bool(), count


def simulate_move_sampled(boards, actions, seed=0x2048, step_index=0, id_base=0):
    """The hybrid agent's simulate_move (agents/hybrid.py:578-629) for every (board, action): up to three sampled empty
    cells x {2, 4}, rewards weighted 0.9 / 0.1. Returns (succ uint8 (n,8,16), reward float64 (n,8), done bool (n,8),
    count uint8 (n,)); only the first count[i] slots of row i are successors."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    L.require_device_tensor(actions, torch.uint8, None, "actions")
    n = boards.shape[0]
    if actions.shape[0] != n:
        raise ValueError("g2048: actions length must equal the number of boards")
    dev = boards.device
    succ = torch.empty((n, 8, 16), dtype=torch.uint8, device=dev)
    reward = torch.empty((n, 8), dtype=torch.float64, device=dev)
    done = torch.empty((n, 8), dtype=torch.uint8, device=dev)
    count = torch.empty(n, dtype=torch.uint8, device=dev)
    L.call(dev, L.lib().g2048_simulate_move_sampled, boards.data_ptr(), actions.data_ptr(), succ.data_ptr(), reward.data_ptr(),
           done.data_ptr(), count.data_ptr(), L.u64(seed), L.u64(step_index), L.u64(id_base), n, L.stream_ptr(dev))
    return succ, reward, done.bool(), count


def pack(tiles, out=None):
    """int32 (n,16) real tile values (the reference's state layout) -> packed codes."""
    L.require_device_tensor(tiles, torch.int32, (16,), "tiles")
    if out is None:
        out = torch.empty((tiles.shape[0], 16), dtype=torch.uint8, device=tiles.device)
    L.call(tiles.device, L.lib().g2048_pack_i32, tiles.data_ptr(), out.data_ptr(), tiles.shape[0], L.stream_ptr(tiles.device))
    return out


def unpack(boards, out=None):
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    if out is None:
        out = torch.empty((boards.shape[0], 16), dtype=torch.int32, device=boards.device)
    L.call(boards.device, L.lib().g2048_unpack_i32, boards.data_ptr(), out.data_ptr(), boards.shape[0], L.stream_ptr(boards.device))
    return out


def synth_boards(n, seed=0x2048, id_base=0, p_empty=0.30, max_code=11, device="cuda", out=None):
    """Synthetic boards of the benchmark configs, generated on the device."""
    if out is None:
        out = torch.empty((n, 16), dtype=torch.uint8, device=device)
    L.require_device_tensor(out, torch.uint8, (16,), "out")
    L.call(out.device, L.lib().g2048_synth_boards, out.data_ptr(), L.u64(seed), L.u64(id_base), out.shape[0],
           int(round(p_empty * 65536)), int(max_code), L.stream_ptr(out.device))
    return out


def synth_actions(n, seed=0x2048, step_index=0, id_base=0, device="cuda", out=None):
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=device)
    L.require_device_tensor(out, torch.uint8, None, "out")
    L.call(out.device, L.lib().g2048_synth_actions, out.data_ptr(), L.u64(seed), L.u64(step_index), L.u64(id_base), out.shape[0],
                                        L.stream_ptr(out.device))
    return out


def metrics(boards, scores=None, flags=None, expanded=None, out=None):
    """Per-shard metric vector (int64[24]): n, sum(score), #done, sum(expanded), hist of max code 0..17."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    if out is None:
        out = torch.zeros(24, dtype=torch.int64, device=boards.device)
    L.call(boards.device, L.lib().g2048_metrics, boards.data_ptr(), scores.data_ptr() if scores is not None else None,
                                  flags.data_ptr() if flags is not None else None,
                                  expanded.data_ptr() if expanded is not None else None,
                                  out.data_ptr(), boards.shape[0], L.stream_ptr(boards.device))
    return out


class BeamHistory:
    """The caller-owned state of the depth-balanced block order (include/g2048.h, g2048_beam_get_action_hist): the history
    buffer the blocks of one call file their games in for the next call, and the call index. One object serves ONE sequence of
    calls on one stream of one device; `BatchedBeamSearch` owns one, `beam_get_action(balanced_order=True)` keeps one per
    (device, stream) in a small registry. Thread-safe: advancing the index and enqueueing the launch happen under the object's
    lock, so two host threads that share it still hand the library consecutive indices in launch order (the device side
    degrades to caller order on any inconsistency anyway -- results never depend on the order)."""

    def __init__(self, device="cuda"):
        import threading
        self.device = torch.device(device)
        self.lock = threading.Lock()
        self.buf, self.n, self.calls = None, 0, 0

    def _prepare(self, n, need):
        """(buffer, call index) for the next call over n roots; the lock is held by the caller."""
        if self.buf is None or self.buf.numel() < need or self.n != n:
            if self.buf is None or self.buf.numel() < need:
                self.buf = torch.empty(need, dtype=torch.uint8, device=self.device)
            self.buf.zero_()
            self.n, self.calls = n, 0
        self.calls += 1
        if self.calls >= 0x7fffffff:
            self.buf.zero_()
            self.calls = 1
        return self.buf, self.calls


class _PerStream:
    """Scratch kept per (device, stream) for the convenience path of beam_get_action: at most `cap` entries, least recently
    used evicted (a stream handle that is never used again does not pin its buffer for the life of the process)."""

    def __init__(self, cap=16):
        import collections
        import threading
        self.cap, self.lock, self.items = cap, threading.Lock(), collections.OrderedDict()

    def get(self, key, make):
        with self.lock:
            v = self.items.get(key)
            if v is None:
                v = self.items[key] = make()
                while len(self.items) > self.cap:
                    self.items.popitem(last=False)
            else:
                self.items.move_to_end(key)
            return v


class _ScratchBox:
    """One (device, stream)'s scratch buffer and the lock that makes "grow if needed + enqueue" one step."""

    def __init__(self):
        import threading
        self.buf, self.lock = None, threading.Lock()


_BEAM_WS = _PerStream()
_BEAM_HIST = _PerStream()


def _dev_index(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _size_query(dev, fn, n):
    """The library's workspace / history size queries depend on the CURRENT device's compute-unit count: ask with the tensors'
    device current, as the launch itself will run."""
    idx = _dev_index(dev)
    if torch.cuda.current_device() == idx:
        return int(fn(n))
    with torch.cuda.device(idx):
        return int(fn(n))


def beam_get_action(roots, width, depth, valid_mask=None, early_threshold=512, mid_threshold=1024,
                    seed=0x2048, step_index=0, game_id_base=0, fixed_down=False, want_expanded=False, keyblock=None,
                    rank_by_counting=False, balanced_order=True, out=None, history=None):
    """BeamSearchAgent.get_action for every root (agents/beam_search_agent.py:71-181).
    Returns (actions uint8, probs float32[, expanded int32]). balanced_order: from 4096 roots on the blocks take the games in
    a depth-balanced order (same results, shorter launch): True = the order the previous call left behind in `history` (a
    BeamHistory the caller owns; None: one kept per (device, stream), shared by whoever calls on that stream -- safe from any
    host thread; the first call of a sequence runs in caller order), "sort" = an order from this call's own roots (one more
    small launch), False = caller order."""
    L.require_device_tensor(roots, torch.uint8, (16,), "roots")
    n = roots.shape[0]
    if not (1 <= int(width) <= L.BEAM_MAX_WIDTH):
        raise ValueError("g2048: beam width must be in 1..%d" % L.BEAM_MAX_WIDTH)
    if valid_mask is not None:
        L.require_device_tensor(valid_mask, torch.uint8, None, "valid_mask")
        if valid_mask.shape[0] != n:
            raise ValueError("g2048: valid_mask length must equal the number of roots")
    dev = roots.device
    if out is not None:             # (actions, probs, expanded) buffers to reuse, e.g. inside a captured graph
        actions, probs, expanded = out
    else:
        actions = torch.empty(n, dtype=torch.uint8, device=dev)
        probs = torch.empty(n, dtype=torch.float32, device=dev)
        expanded = torch.empty(n, dtype=torch.int32, device=dev) if want_expanded else None
    head = (roots.data_ptr(), valid_mask.data_ptr() if valid_mask is not None else None, actions.data_ptr(), probs.data_ptr(),
            expanded.data_ptr() if expanded is not None else None, int(width), int(depth), int(early_threshold),
            int(mid_threshold))
    tail = (L.u64(game_id_base), n, (L.BEAM_FIXED_DOWN if fixed_down else 0) | (L.BEAM_RANK_BY_COUNTING if rank_by_counting else 0),
            L.stream_ptr(dev))
    if keyblock is not None:
        L.call(dev, L.lib().g2048_beam_get_action_dyn, *head, keyblock.words.data_ptr(), *tail)
    else:
        # the depth-balanced block order of large batches. Default: the order of the PREVIOUS call of the same sequence (its
        # blocks file their games into the history buffer, g2048_beam_get_action_hist -- no launch of its own). With
        # balanced_order="sort" the order comes from this call's own roots (beam_order_kernel, one more launch). Neither while
        # the stream is being captured: the cached tensors must not come from a graph's private pool.
        capturing = torch.cuda.is_current_stream_capturing()
        key = (_dev_index(dev), tail[-1])
        if balanced_order == "sort":
            need = 0 if capturing else _size_query(dev, L.lib().g2048_beam_workspace_bytes, n)
            if need:
                # size check, allocation and enqueue under the entry's own lock: two host threads on one stream can neither
                # replace each other's buffer before the launch nor launch into a buffer another thread just dropped (an entry
                # evicted meanwhile keeps its buffer alive through `ws` until this launch is enqueued; the caching allocator's
                # stream ordering covers the rest, the buffer having been allocated on this stream)
                box = _BEAM_WS.get(key, _ScratchBox)
                with box.lock:
                    ws = box.buf
                    if ws is None or ws.numel() < need:
                        ws = box.buf = torch.empty(need, dtype=torch.uint8, device=dev)
                    L.call(dev, L.lib().g2048_beam_get_action_ws, *head, L.u64(seed), L.u64(step_index), *tail[:-1],
                           ws.data_ptr(), need, tail[-1])
            else:
                L.call(dev, L.lib().g2048_beam_get_action_ws, *head, L.u64(seed), L.u64(step_index), *tail[:-1], None, 0, tail[-1])
        else:
            need = 0 if (not balanced_order or capturing) else _size_query(dev, L.lib().g2048_beam_history_bytes, n)
            if not need:
                L.call(dev, L.lib().g2048_beam_get_action_hist, *head, L.u64(seed), L.u64(step_index), *tail[:-1], None, 0, 0, tail[-1])
            else:
                h = history if history is not None else _BEAM_HIST.get(key, lambda: BeamHistory(dev))
                if _dev_index(h.device) != key[0]:
                    raise ValueError("g2048: this BeamHistory belongs to %s, the roots live on %s" % (h.device, dev))
                with h.lock:        # index + enqueue together: the library wants consecutive indices in launch order
                    buf, call_index = h._prepare(n, need)
                    L.call(dev, L.lib().g2048_beam_get_action_hist, *head, L.u64(seed), L.u64(step_index), *tail[:-1],
                           buf.data_ptr(), need, call_index, tail[-1])
    return (actions, probs, expanded) if (want_expanded or (out is not None and expanded is not None)) else (actions, probs)


def play_games(boards, scores, width, depth, max_moves=5000, early_threshold=512, mid_threshold=1024, seed=0x2048,
               game_id_base=0, fixed_down=False, one_phase=False, rank_by_counting=False, tuning=None, want_actions=False):
    """Every game played to completion in ONE launch (beam get_action -> env step fused per game, reference
    run_evaluation.py:48-69): one wavefront owns a game; helper wavefronts of the same launch search the boards the next
    moves can start from ahead of time, for the games that are left when the chip empties (g2048_beam.hip;
    one_phase=True plays without them -- the games are identical). boards / scores are updated in place. Returns a dict
    of per-game tensors: moves, valid_moves, invalid_moves (int32), milestone_move (int32 (n,8), -1 = never), expanded
    (int64), alive (uint8). tuning = (helpers, games_left, stuck, wait_us): the helper-wavefront parameters given explicitly
    (g2048_play_games_tuned; measurements and tests -- the games are the same for every setting). want_actions: also
    "actions", uint8 (n, max_moves): the move-set of every game, 0xFF from its end on (train.py:51,67,140-142; the input of
    `replay_games`)."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _require_scores(scores)
    n = boards.shape[0]
    if not (1 <= int(width) <= L.BEAM_MAX_WIDTH):
        raise ValueError("g2048: beam width must be in 1..%d" % L.BEAM_MAX_WIDTH)
    dev = boards.device
    out = {
        "moves": torch.zeros(n, dtype=torch.int32, device=dev), "valid_moves": torch.zeros(n, dtype=torch.int32, device=dev),
        "invalid_moves": torch.zeros(n, dtype=torch.int32, device=dev),
        "milestone_move": torch.full((n, 8), -1, dtype=torch.int32, device=dev),
        "expanded": torch.zeros(n, dtype=torch.int64, device=dev), "alive": torch.zeros(n, dtype=torch.uint8, device=dev),
    }
    if want_actions:
        out["actions"] = torch.empty((n, int(max_moves)), dtype=torch.uint8, device=dev)     # (the library fills it with 0xFF)
    # the helpers' request slots: caller-owned scratch, like every other buffer of the interface
    ws_bytes = 0 if one_phase else _size_query(dev, L.lib().g2048_play_games_workspace, n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    args = (boards.data_ptr(), scores.data_ptr(), out["moves"].data_ptr(),
            out["valid_moves"].data_ptr(), out["invalid_moves"].data_ptr(), out["milestone_move"].data_ptr(),
            out["expanded"].data_ptr(), out["alive"].data_ptr(), out["actions"].data_ptr() if want_actions else None,
            int(width), int(depth), int(early_threshold),
            int(mid_threshold), int(max_moves), L.u64(seed), L.u64(game_id_base), n,
            (L.BEAM_FIXED_DOWN if fixed_down else 0) | (L.PLAY_ONE_PHASE if one_phase else 0) |
            (L.BEAM_RANK_BY_COUNTING if rank_by_counting else 0),
            ws.data_ptr() if ws is not None else None, ws_bytes)
    if tuning is not None:
        import ctypes
        t4 = (ctypes.c_uint32 * 4)(*[min(max(int(x), 0), 0xFFFFFFFF) for x in tuning])
        L.call(dev, L.lib().g2048_play_games_tuned, *args, ctypes.cast(t4, ctypes.c_void_p), L.stream_ptr(dev))
    else:
        L.call(dev, L.lib().g2048_play_games_ws, *args, L.stream_ptr(dev))
    return out


PLAY_POLICY_MODES = {"masked": L.PLAY_POLICY_MASKED, "unmasked": L.PLAY_POLICY_UNMASKED, "greedy": L.PLAY_POLICY_GREEDY}
_PLAY_NET_WS = _PerStream()


def _net_game_results(boards, scores, max_moves, max_units, units_name, want_rewards, want_actions):
    """The checks play_policy_games, play_tpolicy_games and play_qnet_games make on what they have in common, and their
    dict of per-game result tensors."""
    n, dev = boards.shape[0], boards.device
    if scores.shape[0] != n:
        raise ValueError("g2048: scores length must equal the number of boards")
    if int(max_moves) < 1:
        raise ValueError("g2048: max_moves must be at least 1")
    if not 0 <= int(max_units) <= 0xFFFFFFFF:
        raise ValueError("g2048: %s must be 0 (auto) or a positive 32-bit count" % units_name)
    out = {
        "moves": torch.zeros(n, dtype=torch.int32, device=dev), "valid_moves": torch.zeros(n, dtype=torch.int32, device=dev),
        "invalid_moves": torch.zeros(n, dtype=torch.int32, device=dev),
        "milestone_move": torch.full((n, 8), -1, dtype=torch.int32, device=dev),
        "alive": torch.zeros(n, dtype=torch.uint8, device=dev),
    }
    if want_rewards:
        out["reward_sum"] = torch.zeros(n, dtype=torch.float64, device=dev)
    if want_actions:
        out["actions"] = torch.empty((n, int(max_moves)), dtype=torch.uint8, device=dev)     # (the library fills it with 0xFF)
    return out


def _play_net_games(fn, workspace_fn, boards, scores, net_args, out, max_moves, tail_args):
    """One g2048_play_*_games call: fn(boards, scores, *net_args, <the result arrays of `out`>, max_moves, *tail_args, workspace,
    workspace bytes, stream), the workspace kept per (device, stream) and grown under its lock."""
    n, dev = boards.shape[0], boards.device
    need = int(workspace_fn(n))
    ptr = lambda k: out[k].data_ptr() if k in out else None      # noqa: E731
    box = _PLAY_NET_WS.get((_dev_index(dev), L.stream_ptr(dev)), _ScratchBox)
    with box.lock:          # grow-if-needed and enqueue as one step (see beam_get_action)
        if box.buf is None or box.buf.numel() < need:
            box.buf = torch.empty(need, dtype=torch.uint8, device=dev)
        L.call(dev, fn, boards.data_ptr(), scores.data_ptr(), *net_args, out["moves"].data_ptr(), out["valid_moves"].data_ptr(),
               out["invalid_moves"].data_ptr(), out["milestone_move"].data_ptr(), ptr("reward_sum"), out["alive"].data_ptr(),
               ptr("actions"), int(max_moves), *tail_args, box.buf.data_ptr(), need, L.stream_ptr(dev))
    return out


def _check_play_opts(precision, mode):
    if precision not in POLICY_PRECISIONS:
        raise ValueError("g2048: precision must be 'f32' or 'bf16'")
    if mode not in PLAY_POLICY_MODES:
        raise ValueError("g2048: mode must be one of %s" % (tuple(PLAY_POLICY_MODES),))


def _check_play_blob(kind, packed, precision, dim_ff, n_layers):
    nb = _net_packed_bytes(kind, precision, dim_ff, n_layers)        # (the size needs no device: a wrong blob is refused anywhere)
    if isinstance(packed, torch.Tensor) and packed.numel() != nb:
        raise ValueError("g2048: packed must be a %s blob of %d bytes (dim_ff %d, %d layers)" % (precision, nb, dim_ff, n_layers))


def _require_games(boards, scores, packed, packed_name="packed"):
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _require_scores(scores)
    L.require_device_tensor(packed, torch.uint8, None, packed_name)


def play_policy_games(boards, scores, actor_packed, precision="f32", max_moves=2000, mode="masked", seed=0x2048, game_id_base=0,
                      want_rewards=True, want_actions=False, max_waves=0):
    """Every game played to the end by the PPO actor in ONE launch (g2048_play_policy_games; train.py:54-90 for mode="masked",
    play.py:44-68 for "unmasked", the argmax over the valid moves for "greedy"). actor_packed: the blob of the weights to play
    with (DevicePolicy.actor.blob(1) for the reference's batch-of-one rule), packed with `precision`. boards / scores are
    updated in place. Returns a dict of per-game tensors: moves, valid_moves, invalid_moves (int32), milestone_move (int32
    (n,8), -1 = never), alive (uint8), with want_rewards "reward_sum" (float64: the env rewards summed in move order) and with
    want_actions "actions" (uint8 (n, max_moves), 0xFF from a game's end on: the input of `replay_games`). max_waves: the
    number of wavefronts, 0 = as many as the chip holds (the games are the same for every value)."""
    _require_games(boards, scores, actor_packed, "actor_packed")
    _check_play_opts(precision, mode)
    if actor_packed.numel() != policy_packed_bytes(precision, 4):
        raise ValueError("g2048: actor_packed must be a %s actor blob of %d bytes" % (precision, policy_packed_bytes(precision, 4)))
    out = _net_game_results(boards, scores, max_moves, max_waves, "max_waves", want_rewards, want_actions)
    opts = POLICY_PRECISIONS[precision] | (PLAY_POLICY_MODES[mode] << L.PLAY_POLICY_MODE_SHIFT)
    return _play_net_games(L.lib().g2048_play_policy_games, L.lib().g2048_play_policy_workspace, boards, scores,
                           (actor_packed.data_ptr(),), out, max_moves,
                           (L.u64(seed), L.u64(game_id_base), boards.shape[0], opts, int(max_waves)))


def play_tpolicy_games(boards, scores, packed, dim_ff, n_layers, precision="f32", max_moves=2000, mode="masked", seed=0x2048,
                       game_id_base=0, want_rewards=True, want_actions=False, max_blocks=0):
    """Every game played to the end by the transformer policy in ONE launch (g2048_play_tpolicy_games): play_policy_games with
    the network of tpolicy_forward. packed: the blob of tpolicy_pack for (precision, dim_ff, n_layers). boards / scores are
    updated in place. Returns play_policy_games' dict of per-game tensors: moves, valid_moves, invalid_moves (int32),
    milestone_move (int32 (n,8), -1 = never), alive (uint8), with want_rewards "reward_sum" (float64) and with want_actions
    "actions" (uint8 (n, max_moves), 0xFF from a game's end on: the input of `replay_games`). max_blocks: the number of
    blocks (16 games in flight each), 0 = as many as the chip holds (the games are the same for every value)."""
    _check_play_opts(precision, mode)
    _check_play_blob("tpolicy", packed, precision, dim_ff, n_layers)
    _require_games(boards, scores, packed)
    out = _net_game_results(boards, scores, max_moves, max_blocks, "max_blocks", want_rewards, want_actions)
    opts = POLICY_PRECISIONS[precision] | (PLAY_POLICY_MODES[mode] << L.PLAY_POLICY_MODE_SHIFT)
    return _play_net_games(L.lib().g2048_play_tpolicy_games, L.lib().g2048_play_tpolicy_workspace, boards, scores,
                           (packed.data_ptr(), int(dim_ff), int(n_layers)), out, max_moves,
                           (L.u64(seed), L.u64(game_id_base), boards.shape[0], opts, int(max_blocks)))


def play_qnet_games(boards, scores, packed, dim_ff, n_layers, precision="f32", max_moves=2000, epsilon=0.0, seed=0x2048,
                    game_id_base=0, want_rewards=True, want_actions=False, max_waves=0):
    """Every game played to the end by the hybrid agent's Q-network in ONE launch (g2048_play_qnet_games; the reference's
    evaluate_agent, hybrid.py:1176-1210): per move qnet_forward, then select_action at `epsilon` as qnet_select_actions picks
    it (epsilon 0: the exploit action), then the env step. packed: the blob of qnet_pack for (precision, dim_ff, n_layers).
    boards / scores are updated in place. Returns play_policy_games' dict of per-game tensors: moves, valid_moves,
    invalid_moves (int32), milestone_move (int32 (n,8), -1 = never), alive (uint8), with want_rewards "reward_sum" (float64)
    and with want_actions "actions" (uint8 (n, max_moves), 0xFF from a game's end on: the input of `replay_games`).
    max_waves: the number of wavefronts (32 games in flight each), 0 = as many as the chip holds (the games are the same for
    every value)."""
    _check_play_blob("qnet", packed, precision, dim_ff, n_layers)
    epsilon = float(epsilon)
    if not 0.0 <= epsilon <= 1.0:
        raise ValueError("g2048: epsilon must lie in [0, 1]")
    _require_games(boards, scores, packed)
    out = _net_game_results(boards, scores, max_moves, max_waves, "max_waves", want_rewards, want_actions)
    return _play_net_games(L.lib().g2048_play_qnet_games, L.lib().g2048_play_qnet_workspace, boards, scores,
                           (packed.data_ptr(), int(dim_ff), int(n_layers)), out, max_moves,
                           (epsilon, L.u64(seed), L.u64(game_id_base), boards.shape[0], POLICY_PRECISIONS[precision], int(max_waves)))


def play_qnet_beam_games(boards, scores, packed, dim_ff, n_layers, precision="f32", max_moves=2000, epsilon=0.0, beam_width=15,
                         search_depth=30, threshold=64, seed=0x2048, game_id_base=0, want_rewards=True, want_actions=False, max_waves=0):
    """play_qnet_games with the reference's use_beam_search = True in ONE launch (g2048_play_qnet_beam_games): per move
    qnet_forward, then select_action as qnet_beam_actions picks it at (beam_width, search_depth, threshold), then the env step.
    search_depth >= 2 only (the search then consults no network); search_depth 1 is played move by move
    (evaluate_qnet(fused=False)). Arguments and the returned dict are play_qnet_games'."""
    _check_play_blob("qnet", packed, precision, dim_ff, n_layers)
    epsilon = float(epsilon)
    if not 0.0 <= epsilon <= 1.0:
        raise ValueError("g2048: epsilon must lie in [0, 1]")
    _check_beam_settings(beam_width, search_depth, threshold)
    if int(search_depth) == 1:
        raise ValueError("g2048: search_depth 1 asks the network about every candidate and is not played in one launch "
                         "(qnet_beam_expand, qnet_forward, qnet_beam_actions per move: evaluate_qnet(fused=False))")
    _require_games(boards, scores, packed)
    out = _net_game_results(boards, scores, max_moves, max_waves, "max_waves", want_rewards, want_actions)
    return _play_net_games(L.lib().g2048_play_qnet_beam_games, L.lib().g2048_play_qnet_beam_workspace, boards, scores,
                           (packed.data_ptr(), int(dim_ff), int(n_layers)), out, max_moves,
                           (epsilon, int(beam_width), int(search_depth), int(threshold), L.u64(seed), L.u64(game_id_base),
                            boards.shape[0], POLICY_PRECISIONS[precision], int(max_waves)))


def _check_expectimax(depth, early_threshold, mid_threshold):
    if not 1 <= int(depth) <= L.EXPECTIMAX_MAX_DEPTH:
        raise ValueError("g2048: expectimax depth must be 1 .. %d" % L.EXPECTIMAX_MAX_DEPTH)
    if int(early_threshold) < 0 or int(mid_threshold) < 0:
        raise ValueError("g2048: the phase thresholds are tile values and cannot be negative")


def expectimax_actions(boards, depth=2, mask=None, want_values=False, early_threshold=512, mid_threshold=1024, actions=None, values=None):
    """The expectimax agent's decision for every board (g2048_expectimax_actions, include/g2048_search.h): the valid action with
    the largest expectation over ALL spawn successors (tile 2 with 0.9, tile 4 with 0.1) of the value `depth` plies down, the
    leaves valued by the beam agent's heuristic; env moves, ties to the lowest action, 0 where no move is left. mask: optional
    uint8 (n,), bit a = action a may be chosen (ANDed with the env's valid moves). Returns actions (uint8 (n,)), or with
    want_values (or a `values` tensor) the pair (actions, values): float64 (n,4), -inf for a move that is invalid or masked out.
    One launch, one wavefront per board; the f64 sums are taken in a fixed order, so the bits do not depend on the launch."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _check_expectimax(depth, early_threshold, mid_threshold)
    n, dev = boards.shape[0], boards.device
    if mask is not None:
        L.require_device_tensor(mask, torch.uint8, None, "mask")
        if mask.numel() != n:
            raise ValueError("g2048: mask must have one byte per board")
    actions = _output(actions, n, torch.uint8, (), "actions", dev)
    if want_values or values is not None:
        values = _output(values, n, torch.float64, (4,), "values", dev)
    L.search_call(dev, L.search_lib().g2048_expectimax_actions, boards.data_ptr(), mask.data_ptr() if mask is not None else None,
                  actions.data_ptr(), values.data_ptr() if values is not None else None, int(depth), int(early_threshold),
                  int(mid_threshold), n, L.stream_ptr(dev))
    return (actions, values) if values is not None else actions


def play_expectimax_games(boards, scores, depth=2, max_moves=5000, early_threshold=512, mid_threshold=1024, seed=0x2048, game_id_base=0,
                          want_rewards=True, want_actions=False, max_waves=0):
    """Every game played to the end by the expectimax agent in ONE launch (g2048_play_expectimax_games): per move the decision of
    expectimax_actions at `depth` (no mask), then the env step. boards / scores are updated in place. Returns
    play_policy_games' dict of per-game tensors: moves, valid_moves, invalid_moves (int32), milestone_move (int32 (n,8), -1 =
    never), alive (uint8), with want_rewards "reward_sum" (float64) and with want_actions "actions" (uint8 (n, max_moves), 0xFF
    from a game's end on: the input of `replay_games`). max_waves: the number of wavefronts (one game in flight each), 0 = as
    many as the chip holds (the games are the same for every value)."""
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _require_scores(scores)
    _check_expectimax(depth, early_threshold, mid_threshold)
    out = _net_game_results(boards, scores, max_moves, max_waves, "max_waves", want_rewards, want_actions)
    n, dev = boards.shape[0], boards.device
    lib = L.search_lib()
    need = int(lib.g2048_play_expectimax_workspace(n))
    ptr = lambda k: out[k].data_ptr() if k in out else None      # noqa: E731
    box = _PLAY_NET_WS.get((_dev_index(dev), L.stream_ptr(dev)), _ScratchBox)
    with box.lock:          # grow-if-needed and enqueue as one step (see beam_get_action)
        if box.buf is None or box.buf.numel() < need:
            box.buf = torch.empty(need, dtype=torch.uint8, device=dev)
        L.search_call(dev, lib.g2048_play_expectimax_games, boards.data_ptr(), scores.data_ptr(), int(depth), int(early_threshold),
                      int(mid_threshold), out["moves"].data_ptr(), out["valid_moves"].data_ptr(), out["invalid_moves"].data_ptr(),
                      out["milestone_move"].data_ptr(), ptr("reward_sum"), out["alive"].data_ptr(), ptr("actions"), int(max_moves),
                      L.u64(seed), L.u64(game_id_base), n, int(max_waves), box.buf.data_ptr(), need, L.stream_ptr(dev))
    return out


def replay_games(boards0, actions, n_moves, seed, game_ids=None, game_id_base=0, scores0=None, longest=None):
    """Recorded games replayed into their per-move histories (g2048_replay_games; reference evaluate_beam_search.py:44-50,
    :72-75: board_history / scores_history / max_tiles_history of run_game). boards0 uint8 (k,16): where each game started;
    actions uint8 (k, stride): its action bytes as `play_games(want_actions=True)` wrote them; n_moves int32 (k,); game_ids
    int64 (k,) = the GLOBAL ids the games were played under (None: game_id_base + row). Returns (boards_hist uint8
    (k, L+1, 16), score_hist int32 (k, L+1), flags_hist uint8 (k, L+1)), L = the longest game; entry t = the state before move
    t, entry n_moves = the final state; entries past a game's end are zero. longest: an upper bound of n_moves the caller
    already knows (e.g. the move cap) -- without it the histories are sized by one read-back of n_moves.max()."""
    L.require_device_tensor(boards0, torch.uint8, (16,), "boards0")
    L.require_device_tensor(actions, torch.uint8, None, "actions")
    L.require_device_tensor(n_moves, torch.int32, None, "n_moves")
    k, dev = boards0.shape[0], boards0.device
    if actions.dim() != 2 or actions.shape[0] != k or n_moves.shape[0] != k:
        raise ValueError("g2048: actions must be (k, stride) and n_moves (k,) for k start boards")
    if game_ids is not None:
        L.require_device_tensor(game_ids, torch.int64, None, "game_ids")
        if game_ids.shape[0] != k:
            raise ValueError("g2048: game_ids must have one id per game")
    if scores0 is not None:
        _require_scores(scores0)
    if longest is None:
        longest = int(n_moves.max().item()) if k else 0                          # (one host sync: the histories are sized by it)
    longest = min(int(longest), actions.shape[1])
    hist = longest + 1
    boards_hist = torch.zeros((k, hist, 16), dtype=torch.uint8, device=dev)
    score_hist = torch.zeros((k, hist), dtype=torch.int32, device=dev)
    flags_hist = torch.zeros((k, hist), dtype=torch.uint8, device=dev)
    L.call(dev, L.lib().g2048_replay_games, boards0.data_ptr(), scores0.data_ptr() if scores0 is not None else None,
           game_ids.data_ptr() if game_ids is not None else None, L.u64(game_id_base), actions.data_ptr(), actions.shape[1],
           n_moves.data_ptr(), boards_hist.data_ptr(), score_hist.data_ptr(), flags_hist.data_ptr(), hist, L.u64(seed), k,
           L.stream_ptr(dev))
    return boards_hist, score_hist, flags_hist


def env_step(board, score, record, seed, index, board_id=0, action=0, op=None):
    """One iteration of ONE env in one launch (g2048_env_step): op ENV_OP_STEP (default) / ENV_OP_RESET / ENV_OP_PEEK. board uint8
    (1,16) and score int32 (1,) are updated in place; `record` -- uint8 (80,), device memory or pinned host memory -- receives
    the state as int32 tiles, the score, the flags, the next valid-move mask and the f64 reward (include/g2048.h)."""
    L.require_device_tensor(board, torch.uint8, (16,), "board")
    _require_scores(score)
    if not isinstance(record, torch.Tensor) or record.dtype != torch.uint8 or record.numel() < L.ENV_RECORD_BYTES or not record.is_contiguous():
        raise TypeError("g2048: record must be a contiguous uint8 tensor of at least %d bytes" % L.ENV_RECORD_BYTES)
    if not (record.is_cuda or record.is_pinned()):
        raise RuntimeError("g2048: record must live in device memory or in pinned host memory")
    dev = board.device
    L.call(dev, L.lib().g2048_env_step, board.data_ptr(), score.data_ptr(), int(action) & 0xFFFFFFFF,
           L.ENV_OP_STEP if op is None else int(op), record.data_ptr(), L.u64(seed), L.u64(index), L.u64(board_id), L.stream_ptr(dev))


def minibatch_gather(obs, actions, log_probs, rewards, next_boards, flags, batch, seed, sample_index, want_indices=False, out=None):
    """PPOMemory.sample + the head of PPOAgent.update (agents/ppo_agent.py:21-50, :342-354) on a device-resident trajectory
    (g2048_minibatch_gather): `batch` distinct transitions drawn and gathered by one launch, no host sync. Inputs are flat over
    the transitions: obs (n,16) float32 / float16 / bfloat16, actions uint8, log_probs float32, rewards float32 or float64,
    next_boards uint8 (n,16) (before any auto-reset), flags uint8. Returns dict(states, actions, old_log_probs, rewards,
    next_states, dones[, indices]). out: the dict a previous call of the same batch size returned, to be overwritten (at the
    reference's batch sizes a call is mostly the host time of allocating six small tensors)."""
    if obs.dtype not in _OBS_KIND:
        raise TypeError("g2048: obs must be float32, float16 or bfloat16")
    L.require_device_tensor(obs, obs.dtype, (16,), "obs")
    n, dev = obs.shape[0], obs.device
    L.require_device_tensor(actions, torch.uint8, None, "actions")
    L.require_device_tensor(log_probs, torch.float32, None, "log_probs")
    if rewards.dtype not in (torch.float32, torch.float64):
        raise TypeError("g2048: rewards must be float32 or float64")
    L.require_device_tensor(rewards, rewards.dtype, None, "rewards")
    L.require_device_tensor(next_boards, torch.uint8, (16,), "next_boards")
    L.require_device_tensor(flags, torch.uint8, None, "flags")
    if not (actions.shape[0] == log_probs.shape[0] == rewards.shape[0] == next_boards.shape[0] == flags.shape[0] == n):
        raise ValueError("g2048: all trajectory arrays must have one entry per transition")
    batch = min(int(batch), n)                      # PPOMemory.sample: a batch larger than the buffer is the whole buffer
    if out is not None:
        if out["actions"].shape[0] != batch or out["states"].device != dev or (want_indices and "indices" not in out):
            raise ValueError("g2048: `out` must come from a call with the same batch size, device and want_indices")
        want_indices = "indices" in out
    else:
        out = {"states": torch.empty((batch, 16), dtype=torch.float32, device=dev),
               "actions": torch.empty(batch, dtype=torch.int64, device=dev),
               "old_log_probs": torch.empty(batch, dtype=torch.float32, device=dev),
               "rewards": torch.empty(batch, dtype=torch.float32, device=dev),
               "next_states": torch.empty((batch, 16), dtype=torch.float32, device=dev),
               "dones": torch.empty(batch, dtype=torch.float32, device=dev)}
        if want_indices:
            out["indices"] = torch.empty(batch, dtype=torch.int64, device=dev)
    L.call(dev, L.lib().g2048_minibatch_gather, obs.data_ptr(), _OBS_KIND[obs.dtype], actions.data_ptr(), log_probs.data_ptr(),
           rewards.data_ptr(), int(rewards.dtype == torch.float64), next_boards.data_ptr(), flags.data_ptr(), n, batch, L.u64(seed),
           L.u64(sample_index), out["states"].data_ptr(), out["actions"].data_ptr(), out["old_log_probs"].data_ptr(),
           out["rewards"].data_ptr(), out["next_states"].data_ptr(), out["dones"].data_ptr(),
           out["indices"].data_ptr() if want_indices else None, L.stream_ptr(dev))
    return out


# ---- the hybrid agent's prioritized replay (include/g2048.h, "prioritized experience replay") ---------------------------------
def per_update_workspace_bytes(capacity):
    return int(L.lib().g2048_per_update_workspace(int(capacity)))


def per_sample_workspace_bytes(size, batch=0):
    return int(L.lib().g2048_per_sample_workspace(int(size), int(batch)))


def _per_workspace(t, nbytes, device):
    """A workspace of at least nbytes: allocated when t is None (float64, so that it is 16-byte aligned), else checked."""
    if t is None:
        return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()) or t.numel() * t.element_size() < nbytes:
        raise ValueError("g2048: workspace must be a contiguous device tensor of at least %d bytes" % nbytes)
    return t


def _require_per_buffer(states, next_states, actions, rewards, dones, priorities):
    L.require_device_tensor(states, torch.uint8, (16,), "states")
    L.require_device_tensor(next_states, torch.uint8, (16,), "next_states")
    L.require_device_tensor(actions, torch.uint8, None, "actions")
    L.require_device_tensor(rewards, torch.float32, None, "rewards")
    L.require_device_tensor(dones, torch.uint8, None, "dones")
    L.require_device_tensor(priorities, torch.float32, None, "priorities")
    capacity = priorities.shape[0]
    if not (states.shape[0] == next_states.shape[0] == actions.shape[0] == rewards.shape[0] == dones.shape[0] == capacity):
        raise ValueError("g2048: all arrays of a replay buffer must have one entry per slot")
    return capacity


def per_push(states, next_states, actions, rewards, dones, priorities, size, head, boards, actions_in, rewards_in, next_boards, flags,
             workspace=None):
    """m calls of PrioritizedReplayBuffer.push (agents/hybrid.py:736-740) in order into the ring (g2048_per_push). The six ring
    arrays have `capacity` slots; boards / next_boards uint8 (m,16), actions_in uint8, rewards_in float32 or float64, flags uint8
    (bit 0 = done). Returns the (size, head) after the push."""
    capacity = _require_per_buffer(states, next_states, actions, rewards, dones, priorities)
    dev = priorities.device
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    L.require_device_tensor(next_boards, torch.uint8, (16,), "next_boards")
    L.require_device_tensor(actions_in, torch.uint8, None, "actions")
    if rewards_in.dtype not in (torch.float32, torch.float64):
        raise TypeError("g2048: rewards must be float32 or float64")
    L.require_device_tensor(rewards_in, rewards_in.dtype, None, "rewards")
    L.require_device_tensor(flags, torch.uint8, None, "flags")
    m = boards.shape[0]
    if not (next_boards.shape[0] == actions_in.shape[0] == rewards_in.shape[0] == flags.shape[0] == m):
        raise ValueError("g2048: all arrays of a push must have one entry per transition")
    workspace = _per_workspace(workspace, per_update_workspace_bytes(capacity), dev)
    size, head = int(size), int(head)
    L.call(dev, L.lib().g2048_per_push, states.data_ptr(), next_states.data_ptr(), actions.data_ptr(), rewards.data_ptr(), dones.data_ptr(),
           priorities.data_ptr(), capacity, size, head, boards.data_ptr(), next_boards.data_ptr(), actions_in.data_ptr(),
           rewards_in.data_ptr(), int(rewards_in.dtype == torch.float64), flags.data_ptr(), m, workspace.data_ptr(), L.stream_ptr(dev))
    evicted = max(0, size + m - capacity)
    return min(size + m, capacity), (head + evicted) % capacity


def per_sample(states, next_states, actions, rewards, dones, priorities, size, head, alpha, beta, batch, seed=0x2048, sample_index=0,
               u=None, workspace=None, out=None, want_probs=False):
    """PrioritizedReplayBuffer.sample (agents/hybrid.py:742-757) and the head of DQNAgent.train_step (:961-969, :971-1034) on the
    ring (g2048_per_sample), no host round trip. u: None (counter draws of (seed, REPLAY, sample_index)) or float64 (batch,) on
    the device. Returns dict(indices, weights, states, actions, rewards, next_states, dones, shaped[, probs]); out: the dict a
    previous call of the same batch size returned, to be overwritten."""
    capacity = _require_per_buffer(states, next_states, actions, rewards, dones, priorities)
    dev = priorities.device
    size, head, batch = int(size), int(head), int(batch)
    if u is not None:
        L.require_device_tensor(u, torch.float64, None, "u")
        if u.shape[0] != batch:
            raise ValueError("g2048: u must have one draw per sample")
    if out is None:
        out = {}
    shapes = (("indices", torch.int64, ()), ("weights", torch.float32, ()), ("states", torch.float32, (16,)), ("actions", torch.int64, ()),
              ("rewards", torch.float32, ()), ("next_states", torch.float32, (16,)), ("dones", torch.float32, ()),
              ("shaped", torch.float32, ()))
    for name, dtype, tail in shapes:
        out[name] = _output(out.get(name), batch, dtype, tail, name, dev)
    if want_probs or "probs" in out:
        out["probs"] = _output(out.get("probs"), size, torch.float32, (), "probs", dev)
    workspace = _per_workspace(workspace, per_sample_workspace_bytes(size, batch), dev)
    L.call(dev, L.lib().g2048_per_sample, states.data_ptr(), next_states.data_ptr(), actions.data_ptr(), rewards.data_ptr(), dones.data_ptr(),
           priorities.data_ptr(), capacity, size, head, float(alpha), float(beta), batch, L.u64(seed), L.u64(sample_index),
           u.data_ptr() if u is not None else None, workspace.data_ptr(), *[out[name].data_ptr() for name, _, _ in shapes],
           out["probs"].data_ptr() if "probs" in out else None, L.stream_ptr(dev))
    return out


def dqn_shape_rewards(states, next_states, rewards, out=None):
    """The reward shaping of DQNAgent.train_step (agents/hybrid.py:971-1034) for n (state, next state, reward) triples
    (g2048_dqn_shape_rewards): boards uint8 (n,16), rewards float32; float32 out, bit for bit the reference's."""
    L.require_device_tensor(states, torch.uint8, (16,), "states")
    L.require_device_tensor(next_states, torch.uint8, (16,), "next_states")
    L.require_device_tensor(rewards, torch.float32, None, "rewards")
    n, dev = states.shape[0], states.device
    if not (next_states.shape[0] == rewards.shape[0] == n):
        raise ValueError("g2048: states, next_states and rewards must have one entry per transition")
    out = _output(out, n, torch.float32, (), "out", dev)
    L.call(dev, L.lib().g2048_dqn_shape_rewards, states.data_ptr(), next_states.data_ptr(), rewards.data_ptr(), n, out.data_ptr(),
           L.stream_ptr(dev))
    return out


def per_update_priorities(priorities, size, head, indices, td_errors, workspace=None):
    """update_priorities(indices, td_errors + 1e-5) (agents/hybrid.py:1063-1064, :759-762) on the ring's priorities
    (g2048_per_update_priorities): logical int64 indices, float32 td errors; of duplicates the latest in the batch wins."""
    L.require_device_tensor(priorities, torch.float32, None, "priorities")
    L.require_device_tensor(indices, torch.int64, None, "indices")
    L.require_device_tensor(td_errors, torch.float32, None, "td_errors")
    if indices.shape[0] != td_errors.shape[0]:
        raise ValueError("g2048: indices and td_errors must have one entry per sample")
    capacity, dev = priorities.shape[0], priorities.device
    workspace = _per_workspace(workspace, per_update_workspace_bytes(capacity), dev)
    L.call(dev, L.lib().g2048_per_update_priorities, priorities.data_ptr(), capacity, int(size), int(head), indices.data_ptr(),
           td_errors.data_ptr(), indices.shape[0], workspace.data_ptr(), L.stream_ptr(dev))


# ---- the hybrid agent's experience collection in one launch (include/g2048_collect.h, libg2048_collect_hip.so) ----------------
def qnet_collect_workspace_bytes(n):
    return int(L.collect_lib().g2048_qnet_collect_workspace(int(n)))


def qnet_collect(boards, scores, moves, packed, dim_ff, n_layers, states, next_states, actions, rewards, dones, priorities, size, head,
                 steps, precision="f32", epsilon=0.0, beam_width=0, search_depth=30, threshold=64, seed=0x2048, step_index0=0, id_base=0,
                 max_episode_steps=0, flags=None, workspace=None):
    """`steps` moves of the n environments (boards uint8 (n,16), scores 32-bit, moves int32: the episodes' move counts, all three
    updated in place) played by the Q-network in ONE launch (g2048_qnet_collect; train_agent's acting loop, hybrid.py:1098-1127),
    every transition written into the replay ring as per_push writes a push of steps x n rows. Per step and environment:
    qnet_forward, qnet_select_actions at `epsilon` (beam_width 0) or qnet_beam_actions at (beam_width, search_depth >= 2,
    threshold), step() without options, the ring entry, and a fresh board (step(auto_reset=True)'s) when the step ended the game
    or the episode reached max_episode_steps (0: no cap; the stored done stays 0 then). packed: the blob of qnet_pack for
    (precision, dim_ff, n_layers). flags: uint8 (steps, n), every step's flags byte. Returns (size, head, flags): the ring's size
    and head after the call."""
    _check_play_blob("qnet", packed, precision, dim_ff, n_layers)
    if precision not in POLICY_PRECISIONS:
        raise ValueError("g2048: precision must be 'f32' or 'bf16'")
    epsilon, steps, beam_width = float(epsilon), int(steps), int(beam_width)
    if not 0.0 <= epsilon <= 1.0:
        raise ValueError("g2048: epsilon must lie in [0, 1]")
    if beam_width:
        _check_beam_settings(beam_width, search_depth, threshold)
        if int(search_depth) == 1:
            raise ValueError("g2048: search_depth 1 asks the network about every candidate and is not collected in one launch "
                             "(DQNCollector.collect(fused=False))")
    if steps < 1:
        raise ValueError("g2048: steps must be at least 1")
    if int(max_episode_steps) < 0:
        raise ValueError("g2048: max_episode_steps must be 0 (no cap) or positive")
    capacity = _require_per_buffer(states, next_states, actions, rewards, dones, priorities)
    _require_games(boards, scores, packed)
    L.require_device_tensor(moves, torch.int32, None, "moves")
    n, dev = boards.shape[0], boards.device
    if scores.shape[0] != n or moves.shape[0] != n:
        raise ValueError("g2048: scores and moves must have one entry per board")
    size, head = int(size), int(head)
    if steps * n > capacity:
        raise ValueError("g2048: steps x n = %d x %d transitions exceed the buffer's capacity of %d" % (steps, n, capacity))
    if flags is None:
        flags = torch.empty((steps, n), dtype=torch.uint8, device=dev)
    L.require_device_tensor(flags, torch.uint8, None, "flags")
    if tuple(flags.shape) != (steps, n):
        raise ValueError("g2048: flags must have shape (steps, n)")
    workspace = _per_workspace(workspace, qnet_collect_workspace_bytes(n), dev)
    L.collect_call(dev, L.collect_lib().g2048_qnet_collect, boards.data_ptr(), scores.data_ptr(), moves.data_ptr(), packed.data_ptr(),
                   int(dim_ff), int(n_layers), POLICY_PRECISIONS[precision], epsilon, beam_width, int(search_depth), int(threshold),
                   L.u64(seed), L.u64(step_index0), L.u64(id_base), n, steps, int(max_episode_steps), states.data_ptr(),
                   next_states.data_ptr(), actions.data_ptr(), rewards.data_ptr(), dones.data_ptr(), priorities.data_ptr(), capacity, size,
                   head, flags.data_ptr(), workspace.data_ptr(), L.stream_ptr(dev))
    m = steps * n
    evicted = max(0, size + m - capacity)
    return min(size + m, capacity), (head + evicted) % capacity, flags


# ---- the PPO agent's experience collection in one launch (include/g2048_ppo_collect.h, libg2048_ppo_collect_hip.so) ------------
def ppo_collect(boards, scores, actor_packed, critic_packed=None, steps=1, precision="f32", seed=0x2048, step_index0=0, id_base=0, *,
                actions=None, prob=None, reward=None, flags=None, value=None, obs=None, mask=None, next_boards=None,
                state_maxcode=None, step_counter=None):
    """`steps` moves of the n environments (boards uint8 (n,16) and scores 32-bit, both updated in place) played by the PPO actor in
    ONE launch (g2048_ppo_collect; the acting loop of train.py:55-90). Per step t and environment: policy_forward of the board it
    holds with the blobs of policy_pack for `precision`, then rollout_step(auto_reset=True) without a mask input, at step index
    step_index0 (+ step_counter, an int64 device tensor read inside the kernel) + t. actions, prob (the probability, not its
    log), reward (float32 or float64), flags, and value (with critic_packed) are (steps, n), allocated when None. The optional
    outputs are written only when given: obs (steps + 1, n, 16) float32 / float16 / bfloat16 and mask uint8 (steps + 1, n), whose
    row t is the observation and the env valid-move mask of the board step t acts in (row `steps`: the board the call ends on);
    next_boards uint8 (steps, n, 16), the boards before any reset; state_maxcode uint8 (steps, n).
    Returns (actions, prob, reward, flags, value)."""
    if precision not in POLICY_PRECISIONS:
        raise ValueError("g2048: precision must be 'f32' or 'bf16'")
    steps = int(steps)
    if steps < 1:
        raise ValueError("g2048: steps must be at least 1")
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _require_scores(scores)
    n, dev = boards.shape[0], boards.device
    if scores.shape[0] != n:
        raise ValueError("g2048: scores must have one entry per board")
    for name, blob, n_out in (("actor_packed", actor_packed, 4), ("critic_packed", critic_packed, 1)):
        if blob is None and n_out == 1:
            continue
        L.require_device_tensor(blob, torch.uint8, None, name)
        if blob.numel() != policy_packed_bytes(precision, n_out):
            raise ValueError("g2048: %s must be the blob of policy_pack for precision %r" % (name, precision))
    if value is not None and critic_packed is None:
        raise ValueError("g2048: value needs critic_packed")

    def rows(t, dtype, name, tail=(), extra=0, optional=False):
        shape = (steps + extra, n) + tail
        if t is None:
            return None if optional else torch.empty(shape, dtype=dtype, device=dev)
        L.require_device_tensor(t, dtype, None, name)
        if tuple(t.shape) != shape:
            raise ValueError("g2048: %s must have shape %s (got %s)" % (name, shape, tuple(t.shape)))
        return t

    actions = rows(actions, torch.uint8, "actions")
    prob = rows(prob, torch.float32, "prob")
    if reward is not None and reward.dtype not in (torch.float32, torch.float64):
        raise TypeError("g2048: reward must be float32 or float64")
    reward = rows(reward, torch.float32 if reward is None else reward.dtype, "reward")
    flags = rows(flags, torch.uint8, "flags")
    value = rows(value, torch.float32, "value", optional=critic_packed is None)
    if obs is not None and obs.dtype not in _OBS_KIND:
        raise TypeError("g2048: obs must be float32, float16 or bfloat16")
    obs = rows(obs, None if obs is None else obs.dtype, "obs", (16,), 1, optional=True)
    mask = rows(mask, torch.uint8, "mask", (), 1, optional=True)
    next_boards = rows(next_boards, torch.uint8, "next_boards", (16,), optional=True)
    state_maxcode = rows(state_maxcode, torch.uint8, "state_maxcode", optional=True)
    if step_counter is not None:
        L.require_device_tensor(step_counter, torch.int64, None, "step_counter")
    opts = (L.STEP_REWARD_F64 if reward.dtype == torch.float64 else 0) | L.STEP_AUTO_RESET
    opts |= (_OBS_KIND[obs.dtype] << L.ROLLOUT_OBS_SHIFT) if obs is not None else 0
    opts |= POLICY_PRECISIONS[precision] << L.PPO_COLLECT_PRECISION_SHIFT
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    L.ppo_collect_call(dev, L.ppo_collect_lib().g2048_ppo_collect, boards.data_ptr(), scores.data_ptr(), actor_packed.data_ptr(),
                       ptr(critic_packed), actions.data_ptr(), prob.data_ptr(), reward.data_ptr(), flags.data_ptr(), ptr(value), ptr(obs),
                       ptr(mask), ptr(next_boards), ptr(state_maxcode), L.u64(seed), L.u64(step_index0), ptr(step_counter),
                       L.u64(id_base), n, steps, opts, L.stream_ptr(dev))
    return actions, prob, reward, flags, value


# ---- the transformer policy's experience collection in one launch (include/g2048_tpolicy_collect.h, libg2048_tpolicy_collect_hip.so)
def tpolicy_collect(boards, scores, packed, dim_ff, n_layers, steps=1, precision="f32", seed=0x2048, step_index0=0, id_base=0, *,
                    actions=None, prob=None, reward=None, flags=None, value=None, obs=None, mask=None, next_boards=None,
                    state_maxcode=None, step_counter=None, want_value=True):
    """`steps` moves of the n environments (boards uint8 (n,16) and scores 32-bit, both updated in place) played by the transformer
    policy in ONE launch (g2048_tpolicy_collect). Per step t and environment: tpolicy_forward of the board it holds with `packed`
    (the blob of tpolicy_pack for dim_ff, n_layers and `precision`), then rollout_step(auto_reset=True) without a mask input, at
    step index step_index0 (+ step_counter, an int64 device tensor read inside the kernel) + t. actions, prob (the probability,
    not its log), reward (float32 or float64), flags and value are (steps, n), allocated when None; with want_value=False and no
    value tensor the values are not written and None is returned in their place. The optional outputs are written only when
    given: obs (steps + 1, n, 16) float32 / float16 / bfloat16 and mask uint8 (steps + 1, n), whose row t is the observation and
    the env valid-move mask of the board step t acts in (row `steps`: the board the call ends on); next_boards uint8 (steps, n,
    16), the boards before any reset; state_maxcode uint8 (steps, n).
    Returns (actions, prob, reward, flags, value)."""
    if precision not in POLICY_PRECISIONS:
        raise ValueError("g2048: precision must be 'f32' or 'bf16'")
    steps = int(steps)
    if steps < 1:
        raise ValueError("g2048: steps must be at least 1")
    L.require_device_tensor(boards, torch.uint8, (16,), "boards")
    _require_scores(scores)
    n, dev = boards.shape[0], boards.device
    if scores.shape[0] != n:
        raise ValueError("g2048: scores must have one entry per board")
    _check_blob("tpolicy", packed, precision, dim_ff, n_layers)

    def rows(t, dtype, name, tail=(), extra=0, optional=False):
        shape = (steps + extra, n) + tail
        if t is None:
            return None if optional else torch.empty(shape, dtype=dtype, device=dev)
        L.require_device_tensor(t, dtype, None, name)
        if tuple(t.shape) != shape:
            raise ValueError("g2048: %s must have shape %s (got %s)" % (name, shape, tuple(t.shape)))
        return t

    actions = rows(actions, torch.uint8, "actions")
    prob = rows(prob, torch.float32, "prob")
    if reward is not None and reward.dtype not in (torch.float32, torch.float64):
        raise TypeError("g2048: reward must be float32 or float64")
    reward = rows(reward, torch.float32 if reward is None else reward.dtype, "reward")
    flags = rows(flags, torch.uint8, "flags")
    value = rows(value, torch.float32, "value", optional=not want_value)
    if obs is not None and obs.dtype not in _OBS_KIND:
        raise TypeError("g2048: obs must be float32, float16 or bfloat16")
    obs = rows(obs, None if obs is None else obs.dtype, "obs", (16,), 1, optional=True)
    mask = rows(mask, torch.uint8, "mask", (), 1, optional=True)
    next_boards = rows(next_boards, torch.uint8, "next_boards", (16,), optional=True)
    state_maxcode = rows(state_maxcode, torch.uint8, "state_maxcode", optional=True)
    if step_counter is not None:
        L.require_device_tensor(step_counter, torch.int64, None, "step_counter")
    opts = (L.STEP_REWARD_F64 if reward.dtype == torch.float64 else 0) | L.STEP_AUTO_RESET
    opts |= (_OBS_KIND[obs.dtype] << L.ROLLOUT_OBS_SHIFT) if obs is not None else 0
    opts |= POLICY_PRECISIONS[precision] << L.TPOLICY_COLLECT_PRECISION_SHIFT
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    L.tpolicy_collect_call(dev, L.tpolicy_collect_lib().g2048_tpolicy_collect, boards.data_ptr(), scores.data_ptr(), packed.data_ptr(),
                           int(dim_ff), int(n_layers), actions.data_ptr(), prob.data_ptr(), reward.data_ptr(), flags.data_ptr(), ptr(value),
                           ptr(obs), ptr(mask), ptr(next_boards), ptr(state_maxcode), L.u64(seed), L.u64(step_index0), ptr(step_counter),
                           L.u64(id_base), n, steps, opts, L.stream_ptr(dev))
    return actions, prob, reward, flags, value


PPO_TRUNK_FLOATS, PPO_RUNNING_FLOATS = 46272, 768


def ppo_plain_floats(n_out):
    """Floats of one PPO network's plain parameter (and gradient) buffer: 46272 + 65 n_out, n_out 4 (actor) or 1 (critic)."""
    if n_out not in (4, 1):
        raise ValueError("g2048: n_out must be 4 (actor) or 1 (critic)")
    return PPO_TRUNK_FLOATS + 65 * n_out


def ppo_plain_offsets(n_out):
    """[(name, offset, shape)] of the plain layout (include/g2048.h), in the order of the reference module's named_parameters()."""
    shapes = [("fc1.weight", (256, 16)), ("fc1.bias", (256,)), ("bn1.weight", (256,)), ("bn1.bias", (256,)), ("fc2.weight", (128, 256)),
              ("fc2.bias", (128,)), ("bn2.weight", (128,)), ("bn2.bias", (128,)), ("fc3.weight", (64, 128)), ("fc3.bias", (64,)),
              ("fc4.weight", (n_out, 64)), ("fc4.bias", (n_out,))]
    out, o = [], 0
    for name, shape in shapes:
        out.append((name, o, shape))
        o += shape[0] * (shape[1] if len(shape) == 2 else 1)
    assert o == ppo_plain_floats(n_out)
    return out


PPO_RUNNING_OFFSETS = [("bn1.running_mean", 0, 256), ("bn1.running_var", 256, 256), ("bn2.running_mean", 512, 128),
                       ("bn2.running_var", 640, 128)]


def ppo_train_workspace_bytes(n):
    """Bytes of the workspace the PPO training calls need for n rows (g2048_ppo_train_workspace)."""
    return _sized(L.lib().g2048_ppo_train_workspace(int(n)),
                  "g2048: the PPO training pass takes 1 .. %d rows (the batch statistics are the whole batch's; a larger batch "
                  "is refused, not truncated); got n = %d",
                  L.PPO_BATCH_MAX, int(n))


def _ppo_flat(t, floats, name):
    L.require_device_tensor(t, torch.float32, None, name)
    if t.dim() != 1 or t.numel() != floats:
        raise ValueError("g2048: %s must be a flat float32 tensor of %d floats" % (name, floats))
    return t


def ppo_pair(v, name):
    """(actor's, critic's) of a hyper-parameter given as a scalar or a pair."""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("g2048: %s must be a scalar or an (actor, critic) pair" % name)
        return float(v[0]), float(v[1])
    return float(v), float(v)


def ppo_dropout_p(p, name="dropout"):
    """A dropout probability as the library takes it: a finite float, 0 <= p < 1."""
    p = float(p)
    if not 0.0 <= p < 1.0:              # a NaN fails both comparisons
        raise ValueError("g2048: %s must be finite, 0 <= p < 1 (got %r)" % (name, p))
    return p


def ppo_dropout_mask(n, net, site, p, seed=0, call_index=0, device="cuda", out=None):
    """The keep bits of one dropout site of one call (g2048_ppo_dropout_mask), written through the function the training passes
    draw them with: uint8 (n, F), F = 256 for site 0 (after bn1) and 128 for site 1 (after bn2), net 0 the actor's and 1 the
    critic's, 1 where the element is kept. Element (row, feature) is kept iff rng_draw(rng_keys(seed, 11, call_index),
    ((2 net + site) << 32) | (row F + feature), 0) >= floor(p 2^32); a kept element is multiplied by float32(1 / (1 - p)), a
    dropped one by 0. No synchronisation."""
    if net not in (0, 1) or site not in (0, 1):
        raise ValueError("g2048: net must be 0 (actor) or 1 (critic), site 0 (after bn1) or 1 (after bn2)")
    p, n = ppo_dropout_p(p), int(n)
    if not 0 <= n <= L.PPO_BATCH_MAX:
        raise ValueError("g2048: a dropout mask has 0 .. %d rows (the PPO training pass's batch limit); got n = %d" % (L.PPO_BATCH_MAX, n))
    dev = torch.device(device)
    out = _output(out, n, torch.uint8, (256 if site == 0 else 128,), "out", dev)
    if n:
        L.call(out.device, L.lib().g2048_ppo_dropout_mask, L.u64(seed), L.u64(call_index), net, site, p, out.data_ptr(), n,
               L.stream_ptr(out.device))
    return out


def ppo_forward_train(states, plain, n_out, running=None, out=None, workspace=None, dropout=0.0, seed=0, call_index=0, net=0):
    """One PPO network's TRAINING-mode forward (g2048_ppo_forward_train, with dropout g2048_ppo_forward_train_dropout): BatchNorm
    on batch statistics (skipped for one row, as the reference's forward skips it), then dropout with probability `dropout` after
    each BatchNorm (for one row too), the masks those of ppo_dropout_mask(n, net, site, dropout, seed, call_index); dropout = 0
    is the pass without it, bit for bit. states float32 (n,16); plain: the network's plain float32 parameter buffer
    (ppo_plain_floats(n_out)); running: the 768-float running-statistics buffer, moved by momentum 0.1 when given, untouched
    when None. Returns probabilities float32 (n,4) for n_out 4, values float32 (n,1) for n_out 1. No synchronisation."""
    p = ppo_dropout_p(dropout)
    if net not in (0, 1):
        raise ValueError("g2048: net must be 0 (the actor's masks) or 1 (the critic's)")
    L.require_device_tensor(states, torch.float32, (16,), "states")
    _ppo_flat(plain, ppo_plain_floats(n_out), "plain")
    if running is not None:
        _ppo_flat(running, PPO_RUNNING_FLOATS, "running")
    n, dev = states.shape[0], states.device
    out = _output(out, n, torch.float32, (n_out,), "out", dev)
    if n == 0:
        return out
    workspace = _workspace(workspace, ppo_train_workspace_bytes(n), dev)
    run = running.data_ptr() if running is not None else None
    if p == 0.0:
        L.call(dev, L.lib().g2048_ppo_forward_train, states.data_ptr(), plain.data_ptr(), run, int(n_out), out.data_ptr(), n,
               workspace.data_ptr(), L.stream_ptr(dev))
    else:
        L.call(dev, L.lib().g2048_ppo_forward_train_dropout, states.data_ptr(), plain.data_ptr(), run, int(n_out), net, p, L.u64(seed),
               L.u64(call_index), out.data_ptr(), n, workspace.data_ptr(), L.stream_ptr(dev))
    return out


def ppo_advantages(values, next_values, rewards, dones, gamma=0.995, returns=None, advantages=None):
    """agents/ppo_agent.py:368-373 in one launch (g2048_ppo_advantages): returns = rewards + gamma * next_values * (1 - dones),
    advantages = returns - values, normalised by their mean and unbiased std (+ 1e-8) when there is more than one row. All float32
    (n,) (values and next_values may be (n,1)). Returns (returns, advantages). No synchronisation."""
    values, next_values = (t.reshape(-1) if isinstance(t, torch.Tensor) else t for t in (values, next_values))
    for t, name in ((values, "values"), (next_values, "next_values"), (rewards, "rewards"), (dones, "dones")):
        L.require_device_tensor(t, torch.float32, (), name)
    n, dev = values.shape[0], values.device
    if not (next_values.shape[0] == rewards.shape[0] == dones.shape[0] == n):
        raise ValueError("g2048: values, next_values, rewards and dones must have one entry per row")
    returns = _output(returns, n, torch.float32, (), "returns", dev)
    advantages = _output(advantages, n, torch.float32, (), "advantages", dev)
    if n > L.PPO_BATCH_MAX:
        ppo_train_workspace_bytes(n)                 # raises
    L.call(dev, L.lib().g2048_ppo_advantages, values.data_ptr(), next_values.data_ptr(), rewards.data_ptr(), dones.data_ptr(), float(gamma),
           returns.data_ptr(), advantages.data_ptr(), n, L.stream_ptr(dev))
    return returns, advantages


def ppo_loss_grad(states, actions, old_log_probs, advantages, returns, plain_actor, plain_critic, running_actor=None, running_critic=None,
                  clip_epsilon=0.3, value_coef=0.4, entropy_coef=0.05, grad_actor=None, grad_critic=None, losses=None, workspace=None,
                  dropout=0.0, seed=0, call_index=0):
    """One epoch body of PPOAgent.update (agents/ppo_agent.py:378-400) up to backward() on the device (g2048_ppo_loss_grad, with
    dropout g2048_ppo_loss_grad_dropout): both networks' training-mode forwards (running statistics moved where a buffer is
    given), the clipped-surrogate, value and entropy loss and d loss / d parameter of both networks in their plain layouts,
    OVERWRITTEN, never accumulated into. states float32 (n,16), actions int64 (n,), old_log_probs, advantages, returns float32
    (n,). dropout: a probability or an (actor, critic) pair, applied after each BatchNorm as in ppo_forward_train, both networks'
    masks those of (seed, call_index), the backward regenerating them; 0 is the pass without it, bit for bit. f32 only. An action
    outside 0..3 is the caller's error (the kernel reads actions & 3). No synchronisation. Returns (losses float32 (4,) = loss,
    actor_loss, value_loss, entropy; grad_actor; grad_critic)."""
    p_actor, p_critic = (ppo_dropout_p(p) for p in ppo_pair(dropout, "dropout"))
    L.require_device_tensor(states, torch.float32, (16,), "states")
    L.require_device_tensor(actions, torch.int64, (), "actions")
    for t, name in ((old_log_probs, "old_log_probs"), (advantages, "advantages"), (returns, "returns")):
        L.require_device_tensor(t, torch.float32, (), name)
    n, dev = states.shape[0], states.device
    if not (actions.shape[0] == old_log_probs.shape[0] == advantages.shape[0] == returns.shape[0] == n):
        raise ValueError("g2048: actions, old_log_probs, advantages and returns must have one entry per row")
    _ppo_flat(plain_actor, ppo_plain_floats(4), "plain_actor")
    _ppo_flat(plain_critic, ppo_plain_floats(1), "plain_critic")
    for t, name in ((running_actor, "running_actor"), (running_critic, "running_critic")):
        if t is not None:
            _ppo_flat(t, PPO_RUNNING_FLOATS, name)
    if grad_actor is None:
        grad_actor = torch.empty(ppo_plain_floats(4), dtype=torch.float32, device=dev)
    if grad_critic is None:
        grad_critic = torch.empty(ppo_plain_floats(1), dtype=torch.float32, device=dev)
    _ppo_flat(grad_actor, ppo_plain_floats(4), "grad_actor")
    _ppo_flat(grad_critic, ppo_plain_floats(1), "grad_critic")
    if losses is None:
        losses = torch.empty(4, dtype=torch.float32, device=dev)
    _ppo_flat(losses, 4, "losses")
    if n == 0:
        return losses, grad_actor, grad_critic
    workspace = _workspace(workspace, ppo_train_workspace_bytes(n), dev)
    head = (states.data_ptr(), actions.data_ptr(), old_log_probs.data_ptr(), advantages.data_ptr(), returns.data_ptr(), plain_actor.data_ptr(),
            plain_critic.data_ptr(), running_actor.data_ptr() if running_actor is not None else None,
            running_critic.data_ptr() if running_critic is not None else None, float(clip_epsilon), float(value_coef), float(entropy_coef))
    tail = (n, grad_actor.data_ptr(), grad_critic.data_ptr(), losses.data_ptr(), workspace.data_ptr(), L.stream_ptr(dev))
    if p_actor == 0.0 and p_critic == 0.0:
        L.call(dev, L.lib().g2048_ppo_loss_grad, *head, *tail)
    else:
        L.call(dev, L.lib().g2048_ppo_loss_grad_dropout, *head, p_actor, p_critic, L.u64(seed), L.u64(call_index), *tail)
    return losses, grad_actor, grad_critic


def ppo_step_workspace_bytes():
    """Bytes of the workspace ppo_adam_step needs (g2048_ppo_step_workspace): the scalars its first launch prepares."""
    return L.lib().g2048_ppo_step_workspace()


def ppo_adam_step(plain_actor, grad_actor, exp_avg_actor, exp_avg_sq_actor, plain_critic, grad_critic, exp_avg_critic, exp_avg_sq_critic,
                  counters, losses=None, lr=(8e-4, 2e-3), betas=(0.9, 0.999), eps=1e-8, max_norm=0.5, norms=None, workspace=None):
    """What follows backward() in an epoch of PPOAgent.update (agents/ppo_agent.py:403-416) for both networks in two launches
    (g2048_ppo_adam_step): the NaN check on losses[0], clip_grad_norm_(max_norm) per network and an Adam step per network. The
    eight buffers are flat float32 device tensors of ppo_plain_floats(4) (actor) and ppo_plain_floats(1) (critic) in the plain
    layout, all updated IN PLACE (the gradients are left clipped); counters is int64 (4,) on the device = {actor steps applied,
    critic steps applied, calls skipped for a NaN loss, calls skipped for a gradient norm that is not finite}, and the bias
    correction's step number is taken from it ON THE DEVICE. losses: ppo_loss_grad's float32 (4,) (or any float32 tensor whose
    first element is the loss), None: no loss gate. lr and eps are a scalar or an (actor, critic) pair; max_norm None means no
    clipping. A NaN loss or a norm of either network that is not finite leaves all eight buffers and both step counters untouched.
    No synchronisation. Returns the two gradient norms before clipping, float32 (2,), written on every call."""
    actor, critic = ppo_plain_floats(4), ppo_plain_floats(1)
    buffers = (("plain_actor", plain_actor, actor), ("grad_actor", grad_actor, actor), ("exp_avg_actor", exp_avg_actor, actor),
               ("exp_avg_sq_actor", exp_avg_sq_actor, actor), ("plain_critic", plain_critic, critic), ("grad_critic", grad_critic, critic),
               ("exp_avg_critic", exp_avg_critic, critic), ("exp_avg_sq_critic", exp_avg_sq_critic, critic))
    dev = _step_buffers(buffers)
    _step_counters(counters, 4)
    _gate_losses(losses)
    norms = _float_output(norms, (2,), "norms", dev)
    workspace = _workspace(workspace, ppo_step_workspace_bytes(), dev)
    for t, name in ((counters, "counters"), (losses, "losses"), (norms, "norms"), (workspace, "workspace")):
        if t is not None and t.device != dev:
            raise ValueError("g2048: %s on %s, plain_actor on %s" % (name, t.device, dev))
    (lr_a, lr_c), (eps_a, eps_c) = ppo_pair(lr, "lr"), ppo_pair(eps, "eps")
    L.call(dev, L.lib().g2048_ppo_adam_step, *[t.data_ptr() for _, t, _ in buffers], losses.data_ptr() if losses is not None else None,
           counters.data_ptr(), lr_a, lr_c, float(betas[0]), float(betas[1]), eps_a, eps_c,
           float("inf") if max_norm is None else float(max_norm), norms.data_ptr(), workspace.data_ptr(), L.stream_ptr(dev))
    return norms


def launch_plan(compute_units=0, resident_blocks_per_cu=0, n_games=0):
    """The chip-size arithmetic of the library (g2048_launch_plan; a host function, usable without a GPU when compute_units
    is given): dict(order_row, order_min_games, helper_cap, default_helpers)."""
    import ctypes
    out = (ctypes.c_uint32 * 4)()
    L.check(L.lib().g2048_launch_plan(int(compute_units), int(resident_blocks_per_cu), int(n_games), ctypes.cast(out, ctypes.c_void_p)))
    return dict(order_row=out[0], order_min_games=out[1], helper_cap=out[2], default_helpers=out[3])


def device_plan(width=20, n_games=4096, device="cuda"):
    """What the library asks the current device before a beam / evaluation launch (g2048_device_plan): dict(compute_units,
    play_resident_blocks_per_cu, helper_cap, default_helpers, beam_resident_blocks, beam_issue_priority)."""
    import ctypes
    out = (ctypes.c_uint32 * 6)()
    with torch.cuda.device(torch.device(device)):
        L.check(L.lib().g2048_device_plan(int(width), int(n_games), ctypes.cast(out, ctypes.c_void_p)))
    return dict(compute_units=out[0], play_resident_blocks_per_cu=out[1], helper_cap=out[2], default_helpers=out[3],
                beam_resident_blocks=out[4], beam_issue_priority=bool(out[5]))


def selftest(device="cuda"):
    r = torch.full((1,), 0xFFFF, dtype=torch.int32, device=device)
    L.call(r.device, L.lib().g2048_selftest, r.data_ptr(), L.stream_ptr(r.device))
    return int(r.item())
