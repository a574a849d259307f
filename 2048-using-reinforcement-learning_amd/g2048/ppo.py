"""The reference's PPOAgent.update() (agents/ppo_agent.py:357-416) on the device.

`DevicePPOLearner(actor, critic, clip_epsilon=0.3, value_coef=0.4, entropy_coef=0.05, dropout=0.0, dropout_seed=0)` takes the reference's ActorNetwork /
CriticNetwork layout (attributes fc1..fc4 Linear 16-256-128-64-{4|1}, bn1, bn2 BatchNorm1d, in either mode; anything else raises
ValueError) and evaluates the function update() trains: both networks in TRAINING mode, BatchNorm on batch statistics with its
running statistics moving on every forward (skipped for a batch of one row, as the reference's forward skips it).

Dropout. The reference's networks apply nn.Dropout(0.2) after each BatchNorm (for one row, where the BatchNorms are skipped, after
the two ReLUs), and update() runs them in training mode, the two critic forwards of its no-gradient block included. `dropout`
says what the device pass does with those layers: with 0.0 (the default) they are IGNORED, which is update() with p = 0 and what this
class computed before it knew dropout, bit for bit; a probability, or an (actor, critic) pair, applies it; "module" takes each
module's own `dropout.p` (the reference's 0.2). The masks are not torch's: element (row, feature) of site s (0 after bn1, 1
after bn2) of network w (0 actor, 1 critic) is kept iff one draw of the library's counter RNG (DESIGN.md "RNG", domain 11), a pure
function of (dropout_seed, call index, w, s, row, feature), is at least floor(p 2^32), and a kept element is multiplied by
float32(1 / (1 - p)): the same distribution as torch's, reproducible from the seed and the index (ops.ppo_dropout_mask writes the
keep bits), regenerated in the backward pass instead of stored. `dropout_index` is the call index of the NEXT training-mode
forward, a Python int counted on the host: probs, values and loss_and_grad take one each (both networks of loss_and_grad share it),
advantages two (states, then next states), so update(epochs=E) takes 2 + E. No forward is ever skipped (the NaN gate skips only
the optimiser step), so the count needs nothing from the device. dropout_state() / set_dropout_state() carry (seed, index) through
a checkpoint. The index is a launch scalar: a captured graph of update() replays the SAME masks on every replay. Out of scope:
DevicePolicy and the rollout kernels are eval mode, as get_action uses the networks; bf16. (The hybrid Q-network's eight dropout
sites are DeviceQNetwork(dropout=...)'s, g2048/qnet.py.)

Each network lives in three flat float32 buffers on the modules' device: `plain` (the parameters, layout of include/g2048.h =
the module's named_parameters() order), `grad` (same layout, overwritten by loss_and_grad) and `running` (bn1.running_mean,
bn1.running_var, bn2.running_mean, bn2.running_var). attach_params() makes the modules' parameters and running buffers views
into them, attach_grads() the parameters' .grad: from then on loss_and_grad, clip_grad_norm_, a stock torch.optim.Adam step and
DevicePolicy.refresh() (on the same modules, back in eval mode) form a whole update with no copy.

The end of every epoch (:403-416: the NaN check on the loss, clip_grad_norm_(0.5) per network, an Adam step per network) is
adam_step(): two launches over both networks (g2048_ppo_adam_step), the moments in two more buffers per network (`exp_avg`,
`exp_avg_sq`, laid out like `plain`). update() is the whole sequence: advantages(), then per epoch loss_and_grad and adam_step.
No host decision and no host read is in it, so the rules that the reference decides on the host are decided on the device:

  the skip rules   a call of adam_step changes NOTHING in plain, grad, exp_avg and exp_avg_sq of EITHER network if (1) the loss it
      is given is a NaN (the reference's `if torch.isnan(loss): continue`; isnan only, a +inf loss over finite gradients is
      applied), or else (2) the gradient norm of either network is not finite (stock torch would write NaN into that network's
      weights; an update that reaches one network and not the other is of no use to a caller).
  the counters     `opt_counters`, int64 (4,) on the device: {actor steps applied, critic steps applied, calls skipped by (1),
      calls skipped by (2)}. Adam's bias correction takes its step number from the first two ON THE DEVICE: a skipped call does
      not advance it, as the reference's `continue` does not reach optimizer.step(). The host never learns of a skip unless it
      reads the counters.

Nothing here synchronises with the host (optimizer_state_dict / load_optimizer_state_dict excepted); the outputs are buffers owned
by the learner, one set per (N, stream).
"""
import torch
import torch.nn as nn

from . import ops
from ._encoder_net import OutputCache
from .policy import _Layer, _check_widths

NAME = "DevicePPOLearner"


def parse(module, n_out):
    """The reference-layout module's tensors: (parameters in plain order, [bn1, bn2]). Raises ValueError for anything else."""
    if not isinstance(module, nn.Module):
        raise ValueError("%s: expected a torch.nn.Module, got %s" % (NAME, type(module).__name__))
    names = dict(module.named_children())
    if isinstance(module, nn.Sequential) or not all(k in names for k in ("fc1", "fc2", "fc3", "fc4", "bn1", "bn2")):
        raise ValueError("%s: %s is not the reference's layout (attributes fc1..fc4 and bn1, bn2); no other layout is trained on the "
                         "device" % (NAME, type(module).__name__))
    if not all(isinstance(names["fc%d" % i], nn.Linear) for i in range(1, 5)):
        raise ValueError("%s: fc1..fc4 must be Linear layers" % NAME)
    layers = [_Layer(names["fc%d" % i]) for i in range(1, 5)]
    layers[1].bn_in, layers[2].bn_in = names["bn1"], names["bn2"]
    try:
        _check_widths(layers, n_out)
    except ValueError as e:
        raise ValueError(str(e).replace("DevicePolicy", NAME)) from None
    for bn in (names["bn1"], names["bn2"]):
        if not bn.affine or bn.momentum != 0.1 or bn.eps != 1e-5:
            raise ValueError("%s: the BatchNorms must be affine with momentum 0.1 and eps 1e-5 (the reference's, nn.BatchNorm1d's "
                             "defaults)" % NAME)
    params = []
    for key in ("fc1", "bn1", "fc2", "bn2", "fc3", "fc4"):
        params += [names[key].weight, names[key].bias]
    return params, [names["bn1"], names["bn2"]]


def dropout_of(actor, critic, dropout):
    """(actor's p, critic's p) of DevicePPOLearner's `dropout`: a probability, an (actor, critic) pair, or "module" for each
    module's own `dropout.p`. Raises ValueError for a module without such a layer and for a p outside 0 <= p < 1."""
    if isinstance(dropout, str):
        if dropout != "module":
            raise ValueError("%s: dropout must be a probability, an (actor, critic) pair or \"module\", got %r" % (NAME, dropout))
        layers = [getattr(m, "dropout", None) for m in (actor, critic)]
        if not all(isinstance(d, nn.Dropout) for d in layers):
            raise ValueError("%s: dropout=\"module\" needs an nn.Dropout attribute `dropout` on both modules (the reference's layout)" % NAME)
        dropout = (layers[0].p, layers[1].p)
    try:
        return tuple(ops.ppo_dropout_p(p) for p in ops.ppo_pair(dropout, "dropout"))
    except ValueError as e:
        raise ValueError(str(e).replace("g2048:", NAME + ":")) from None


class _TrainNet:
    """One network's module and its flat buffers: plain, grad, running, and adam_step's exp_avg and exp_avg_sq."""

    def __init__(self, module, n_out):
        self.module, self.n_out = module, n_out
        self.params, self.bns = parse(module, n_out)
        self.device = self.params[0].device
        if self.device.type != "cuda":
            raise RuntimeError("g2048: %s needs the modules on a ROCm device (got %s); there is no CPU path" % (NAME, self.device))
        if any(p.dtype != torch.float32 or p.device != self.device for p in self.params):
            raise ValueError("%s: every parameter must be float32 on one device" % NAME)
        self.offsets = ops.ppo_plain_offsets(n_out)
        floats = ops.ppo_plain_floats(n_out)
        self.plain = torch.empty(floats, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros(floats, dtype=torch.float32, device=self.device)
        self.running = torch.empty(ops.PPO_RUNNING_FLOATS, dtype=torch.float32, device=self.device)
        self.refresh()

    def _running_tensors(self):
        return [self.bns[0].running_mean, self.bns[0].running_var, self.bns[1].running_mean, self.bns[1].running_var]

    @torch.no_grad()
    def refresh(self):
        for p, (_, o, _) in zip(self.params, self.offsets):
            self.plain[o:o + p.numel()].copy_(p.reshape(-1))
        for t, (_, o, k) in zip(self._running_tensors(), ops.PPO_RUNNING_OFFSETS):
            self.running[o:o + k].copy_(t)

    @torch.no_grad()
    def write_back(self):
        for p, (_, o, _) in zip(self.params, self.offsets):
            p.copy_(self.plain[o:o + p.numel()].view(p.shape))
        for t, (_, o, k) in zip(self._running_tensors(), ops.PPO_RUNNING_OFFSETS):
            t.copy_(self.running[o:o + k])

    @torch.no_grad()
    def attach_params(self):
        self.refresh()
        for p, (_, o, _) in zip(self.params, self.offsets):
            p.data = self.plain[o:o + p.numel()].view(p.shape)
        for t, (_, o, k) in zip(self._running_tensors(), ops.PPO_RUNNING_OFFSETS):
            t.data = self.running[o:o + k]

    def attach_grads(self):
        for p, (_, o, _) in zip(self.params, self.offsets):
            p.grad = self.grad[o:o + p.numel()].view(p.shape)

    @property
    def params_attached(self):
        """True while the module's parameters are the views attach_params() made (the first and the last are looked at)."""
        base = self.plain.data_ptr()
        return all(self.params[i].data_ptr() == base + 4 * self.offsets[i][1] for i in (0, -1))

    def _moment(self, key):
        t = self.__dict__.get(key)
        if t is None:
            t = self.__dict__[key] = torch.zeros_like(self.plain)
        return t

    @property
    def exp_avg(self):
        """Adam's first moment of adam_step: float32, laid out like `plain` (zeros, allocated on first use)."""
        return self._moment("_exp_avg")

    @property
    def exp_avg_sq(self):
        """Adam's second moment of adam_step, like exp_avg."""
        return self._moment("_exp_avg_sq")

    def tracked(self, n):
        """What torch's training-mode forward does next to the running statistics: num_batches_tracked += 1, on the device."""
        if n > 1:
            for bn in self.bns:
                bn.num_batches_tracked.add_(1)


def _probs(n, device):
    return torch.empty((n, 4), dtype=torch.float32, device=device)


def _values(n, device):
    return torch.empty((n, 1), dtype=torch.float32, device=device)


def _next_values(n, device):
    return torch.empty((n, 1), dtype=torch.float32, device=device)


def _adv_outputs(n, device):
    return torch.empty(n, dtype=torch.float32, device=device), torch.empty(n, dtype=torch.float32, device=device)


def _losses(n, device):
    return torch.empty(4, dtype=torch.float32, device=device)


def _workspace(n, device):             # refuses n = 0 and n above the maximum
    return torch.empty(ops.ppo_train_workspace_bytes(n), dtype=torch.uint8, device=device)


def _norms(n, device):                 # adam_step's two gradient norms
    return torch.empty(2, dtype=torch.float32, device=device)


def _step_workspace(n, device):
    return torch.empty(ops.ppo_step_workspace_bytes(), dtype=torch.uint8, device=device)


def _update_outputs(epochs, device):   # update()'s losses and norms, a row an epoch
    return torch.empty((epochs, 4), dtype=torch.float32, device=device), torch.empty((epochs, 2), dtype=torch.float32, device=device)


WHICH = ("actor", "critic")


class DevicePPOLearner:
    """PPOAgent.update()'s networks, loss and gradients on the device (module docstring). The hyper-parameters default to the
    reference agent's. dropout, dropout_seed, dropout_index, dropout_state(), set_dropout_state(): the module docstring.

    probs(states) / values(states): one network's training-mode forward on float32 (N,16) observations; the running statistics move
      and num_batches_tracked counts, as in torch.
    advantages(states, next_states, rewards, dones, gamma=0.995) -> (returns, advantages): update()'s no-gradient block (:357-373),
      two training-mode critic forwards (both move the running statistics, as the reference's do) and one launch.
    loss_and_grad(states, actions, old_log_probs, advantages, returns) -> float32 (4,) device tensor (loss, actor_loss, value_loss,
      entropy): one epoch body (:378-400) up to backward(); actor.grad / critic.grad are OVERWRITTEN. A NaN loss is reported, not
      skipped: the reference's `continue` is the caller's decision. Non-finite inputs show as they do in stock torch: the ReLUs,
      the clamps and the minimum pass a NaN on (torch.relu / clamp / min, not fmaxf / fminf), so each loss part is finite, NaN,
      +inf or -inf where stock float32's is (a NaN or -inf old log-prob with advantage 0, a NaN state: a NaN loss), and a
      gradient tensor holds a non-finite value where stock's does. As in stock torch, old_log_probs = -inf under a positive
      advantage gives a FINITE loss over NaN actor gradients (exp's backward, 0 x inf): check the gradients, not the loss alone
      (adam_step does: its second skip rule).
    adam_step(losses=None, lr=(8e-4, 2e-3), max_norm=0.5, betas=(0.9, 0.999), eps=1e-8) -> float32 (2,) device tensor, the two
      gradient norms before clipping: the rest of the epoch body (:403-416) for both networks in two launches; the skip rules and
      opt_counters are in the module docstring.
    update(states, actions, old_log_probs, rewards, next_states, dones, epochs=8, gamma=0.995, **adam_step's) -> (losses
      (epochs,4), norms (epochs,2)): the whole of update() after the sampling, without one host read.
    optimizer_state_dict(which) / load_optimizer_state_dict(which, state_dict), which "actor" or "critic": the moments and the step
      counter in the format of torch.optim.Adam(module.parameters()).state_dict().
    1 <= N <= 4096; states are float32 (N,16) as RolloutCollector.sample returns them, not packed boards."""

    def __init__(self, actor, critic, clip_epsilon=0.3, value_coef=0.4, entropy_coef=0.05, dropout=0.0, dropout_seed=0):
        for v, name in ((clip_epsilon, "clip_epsilon"), (value_coef, "value_coef"), (entropy_coef, "entropy_coef")):
            if not (float(v) >= 0.0 and float(v) != float("inf")):
                raise ValueError("%s: %s must be finite and not negative" % (NAME, name))
        self.clip_epsilon, self.value_coef, self.entropy_coef = float(clip_epsilon), float(value_coef), float(entropy_coef)
        self.dropout = dropout_of(actor, critic, dropout)           # (actor's p, critic's p)
        self.dropout_seed, self.dropout_index = ops.L.u64(dropout_seed), 0
        self.actor, self.critic = _TrainNet(actor, 4), _TrainNet(critic, 1)
        if self.actor.device != self.critic.device:
            raise ValueError("%s: actor and critic live on different devices" % NAME)
        self.device = self.actor.device
        self._out = OutputCache(NAME, self.device)
        self.opt_counters = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._hyper = ((8e-4, 2e-3), (0.9, 0.999), 1e-8)      # the last adam_step's lr, betas, eps: optimizer_state_dict's groups

    def refresh(self):
        """Copies the modules' parameters and running statistics into the buffers (a no-op in effect after attach_params())."""
        self.actor.refresh()
        self.critic.refresh()

    def write_back(self):
        """Copies the buffers into the modules' parameters and running statistics (only needed without attach_params())."""
        self.actor.write_back()
        self.critic.write_back()

    def attach_params(self):
        """Makes every parameter and both BatchNorms' running_mean / running_var of both modules views into the plain and running
        buffers (current values kept): an optimiser, load_state_dict and the device forwards then write through. module.to(...)
        or anything else that gives the tensors new storage undoes it. Returns (actor plain, critic plain)."""
        self.actor.attach_params()
        self.critic.attach_params()
        return self.actor.plain, self.critic.plain

    def attach_grads(self):
        """Makes every parameter's .grad a view into the gradient buffers. Keep the optimiser's zero_grad(set_to_none=False), or
        call attach_grads() again after it. Returns (actor grad, critic grad)."""
        self.actor.attach_grads()
        self.critic.attach_grads()
        return self.actor.grad, self.critic.grad

    def _rows(self, states):
        if not isinstance(states, torch.Tensor) or states.dim() != 2:
            raise TypeError("%s: states must be a float32 (N,16) tensor" % NAME)
        if states.device != self.device:
            raise ValueError("%s: states on %s, weights on %s" % (NAME, states.device, self.device))
        return states.shape[0]

    def dropout_state(self):
        """(dropout_seed, dropout_index): with the weights, what reproduces the masks of every later call."""
        return self.dropout_seed, self.dropout_index

    def set_dropout_state(self, state):
        seed, index = state
        if int(index) < 0:
            raise ValueError("%s: the dropout index must not be negative" % NAME)
        self.dropout_seed, self.dropout_index = ops.L.u64(seed), int(index)

    def _next_index(self):
        index = self.dropout_index
        self.dropout_index = index + 1
        return index

    def _forward(self, net, states, make):
        n = self._rows(states)
        w = 0 if net is self.actor else 1
        out = ops.ppo_forward_train(states, net.plain, net.n_out, running=net.running, out=self._out.get(n, make),
                                    workspace=self._out.get(n, _workspace), dropout=self.dropout[w], seed=self.dropout_seed,
                                    call_index=self._next_index(), net=w)
        net.tracked(n)
        return out

    def probs(self, states):
        return self._forward(self.actor, states, _probs)

    def values(self, states):
        return self._forward(self.critic, states, _values)

    def advantages(self, states, next_states, rewards, dones, gamma=0.995):
        values = self._forward(self.critic, states, _values)
        next_values = self._forward(self.critic, next_states, _next_values)
        returns, adv = self._out.get(values.shape[0], _adv_outputs)
        return ops.ppo_advantages(values, next_values, rewards, dones, gamma, returns=returns, advantages=adv)

    def loss_and_grad(self, states, actions, old_log_probs, advantages, returns):
        return self._loss_and_grad(states, actions, old_log_probs, advantages, returns, None)

    def _loss_and_grad(self, states, actions, old_log_probs, advantages, returns, losses):
        n = self._rows(states)
        losses, _, _ = ops.ppo_loss_grad(states, actions, old_log_probs, advantages, returns, self.actor.plain, self.critic.plain,
                                         self.actor.running, self.critic.running, self.clip_epsilon, self.value_coef, self.entropy_coef,
                                         grad_actor=self.actor.grad, grad_critic=self.critic.grad,
                                         losses=self._out.get(n, _losses) if losses is None else losses, workspace=self._out.get(n, _workspace),
                                         dropout=self.dropout, seed=self.dropout_seed, call_index=self._next_index())
        self.actor.tracked(n)
        self.critic.tracked(n)
        return losses

    def adam_step(self, losses=None, lr=(8e-4, 2e-3), max_norm=0.5, betas=(0.9, 0.999), eps=1e-8):
        """The end of an epoch of update() (ppo_agent.py:403-416) on the device, after loss_and_grad: the NaN check on losses[0]
        (losses: what loss_and_grad returned; None: no check), clip_grad_norm_(max_norm) on each network and an Adam step on each
        network, in two launches over both (g2048_ppo_adam_step). plain is updated IN PLACE from grad (left clipped, as
        clip_grad_norm_ leaves it), the moments are each network's exp_avg and exp_avg_sq. lr and eps are a scalar or an (actor,
        critic) pair, the defaults the reference agent's; max_norm None: no clipping. A NaN loss, or a gradient norm of EITHER
        network that is not finite, skips the call: no buffer of either network changes, and opt_counters[2] or [3] counts it;
        otherwise opt_counters[0] and [1] go up by one, and they are the step numbers of Adam's bias correction, read on the
        device (a skipped call does not advance them). Returns the two norms before clipping, float32 (2,) (the learner's own,
        one per stream; written on a skipped call too), without synchronising. If attach_params() did not make the modules'
        parameters views of the buffers, the call ends with write_back(): the modules equal the buffers bit for bit either way."""
        norms = self._adam_step(losses, lr, max_norm, betas, eps, self._out.get(0, _norms))
        self._plain_changed()
        return norms

    def _adam_step(self, losses, lr, max_norm, betas, eps, norms):
        a, c = self.actor, self.critic
        ops.ppo_adam_step(a.plain, a.grad, a.exp_avg, a.exp_avg_sq, c.plain, c.grad, c.exp_avg, c.exp_avg_sq, self.opt_counters,
                          losses=losses, lr=lr, betas=betas, eps=eps, max_norm=max_norm, norms=norms,
                          workspace=self._out.get(0, _step_workspace))
        self._hyper = (lr, betas, eps)          # as given (ppo_adam_step accepted them); optimizer_state_dict reads them
        return norms

    def _plain_changed(self):
        if not (self.actor.params_attached and self.critic.params_attached):
            self.write_back()

    def update(self, states, actions, old_log_probs, rewards, next_states, dones, epochs=8, gamma=0.995, **adam):
        """PPOAgent.update() after its sampling (ppo_agent.py:357-416) on the device: advantages(states, next_states, rewards,
        dones, gamma), then `epochs` times loss_and_grad and adam_step on that epoch's losses (**adam: adam_step's lr, max_norm,
        betas, eps). A sequence of launches with no host decision and no host read: an epoch whose loss is a NaN or whose
        gradients are not finite is skipped on the device (adam_step) and shows in opt_counters and in the returned rows. Returns
        (losses float32 (epochs,4), norms float32 (epochs,2)), device tensors the learner owns (one pair per (epochs, stream)):
        row e is epoch e's loss_and_grad result and its gradient norms before clipping. DevicePolicy.refresh() stays with the
        caller."""
        epochs = int(epochs)
        if epochs < 1:
            raise ValueError("%s: update needs at least one epoch" % NAME)
        unknown = set(adam) - {"lr", "max_norm", "betas", "eps"}
        if unknown:
            raise TypeError("%s: update got unexpected arguments %s" % (NAME, sorted(unknown)))
        adam = dict(dict(lr=(8e-4, 2e-3), max_norm=0.5, betas=(0.9, 0.999), eps=1e-8), **adam)
        returns, adv = self.advantages(states, next_states, rewards, dones, gamma)
        losses, norms = self._out.get(epochs, _update_outputs)
        for e in range(epochs):
            self._loss_and_grad(states, actions, old_log_probs, adv, returns, losses[e])
            self._adam_step(losses[e], adam["lr"], adam["max_norm"], adam["betas"], adam["eps"], norms[e])
        self._plain_changed()
        return losses, norms

    def _net(self, which):
        if which not in WHICH:
            raise ValueError("%s: which must be 'actor' or 'critic', got %r" % (NAME, which))
        return (self.actor, self.critic)[WHICH.index(which)], WHICH.index(which)

    def optimizer_state_dict(self, which):
        """The state of `which` network's Adam in the format torch.optim.Adam(module.parameters()).state_dict() has: 12 entries in
        named_parameters() order (the plain order), each {step, exp_avg, exp_avg_sq} (copies, shaped like the parameter; step is
        opt_counters' applied-step count), and one parameter group holding the last adam_step's lr, betas and eps for that network
        (the reference agent's before the first call). Before the first applied step the state is empty, as a fresh optimiser's
        is. A stock optimiser's load_state_dict and the reference's save() take it as it is. Synchronises (it reads the
        counter)."""
        net, k = self._net(which)
        lr, betas, eps = self._hyper
        group = torch.optim.Adam([torch.nn.Parameter(torch.zeros(()))], lr=ops.ppo_pair(lr, "lr")[k], betas=(float(betas[0]), float(betas[1])),
                                 eps=ops.ppo_pair(eps, "eps")[k]).state_dict()["param_groups"][0]
        group["params"] = list(range(len(net.params)))
        step, state = int(self.opt_counters[k]), {}
        if step > 0:
            for i, (p, (_, o, _)) in enumerate(zip(net.params, net.offsets)):
                state[i] = dict(step=torch.tensor(float(step)), exp_avg=net.exp_avg[o:o + p.numel()].view(p.shape).clone(),
                                exp_avg_sq=net.exp_avg_sq[o:o + p.numel()].view(p.shape).clone())
        return dict(state=state, param_groups=[group])

    @torch.no_grad()
    def load_optimizer_state_dict(self, which, state_dict):
        """Takes what torch.optim.Adam(module.parameters()).state_dict() (or optimizer_state_dict) gave for `which` network, e.g.
        out of a checkpoint the reference's save() wrote: the moments into exp_avg and exp_avg_sq, the step into opt_counters (the
        skip counts stay). An empty state resets moments and step to 0. The group's lr, betas and eps are NOT taken: they are
        adam_step's arguments. amsgrad, maximize and a weight decay are refused: adam_step is plain Adam."""
        net, k = self._net(which)
        groups, state = state_dict["param_groups"], state_dict["state"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(net.params):
            raise ValueError("%s: expected one parameter group of %d parameters (torch.optim.Adam(module.parameters()))" % (NAME, len(net.params)))
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize") or g.get("weight_decay", 0) != 0:
            raise ValueError("%s: amsgrad, maximize and weight_decay are not what adam_step computes" % NAME)
        if not state:
            net.exp_avg.zero_()
            net.exp_avg_sq.zero_()
            self.opt_counters[k] = 0
            return
        keys = list(g["params"])
        if set(state) != set(keys):
            raise ValueError("%s: the state must hold all %d parameters or none" % (NAME, len(keys)))
        steps = {int(state[key]["step"]) for key in keys}
        if len(steps) != 1 or min(steps) < 0:
            raise ValueError("%s: the parameters' step counts differ or are negative: %s" % (NAME, sorted(steps)))
        for key, p in zip(keys, net.params):
            for name in ("exp_avg", "exp_avg_sq"):
                if tuple(state[key][name].shape) != tuple(p.shape):
                    raise ValueError("%s: %s of parameter %s has shape %s, the parameter %s" % (NAME, name, key, tuple(state[key][name].shape), tuple(p.shape)))
        for key, p, (_, o, _) in zip(keys, net.params, net.offsets):
            net.exp_avg[o:o + p.numel()].copy_(state[key]["exp_avg"].reshape(-1))
            net.exp_avg_sq[o:o + p.numel()].copy_(state[key]["exp_avg_sq"].reshape(-1))
        self.opt_counters[k] = steps.pop()
