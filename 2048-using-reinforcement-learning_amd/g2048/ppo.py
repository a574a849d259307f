"""The gradient half of the reference's PPOAgent.update() (agents/ppo_agent.py:357-400) on the device.

`DevicePPOLearner(actor, critic, clip_epsilon=0.3, value_coef=0.4, entropy_coef=0.05)` takes the reference's ActorNetwork /
CriticNetwork layout (attributes fc1..fc4 Linear 16-256-128-64-{4|1}, bn1, bn2 BatchNorm1d, in either mode; anything else raises
ValueError) and evaluates the function update() trains: both networks in TRAINING mode, BatchNorm on batch statistics with its
running statistics moving on every forward (skipped for a batch of one row, as the reference's forward skips it). The modules'
Dropout layers are IGNORED, as everywhere in this library: the device pass is update() with dropout p = 0.

Each network lives in three flat float32 buffers on the modules' device: `plain` (the parameters, layout of include/g2048.h =
the module's named_parameters() order), `grad` (same layout, overwritten by loss_and_grad) and `running` (bn1.running_mean,
bn1.running_var, bn2.running_mean, bn2.running_var). attach_params() makes the modules' parameters and running buffers views
into them, attach_grads() the parameters' .grad: from then on loss_and_grad, clip_grad_norm_, a stock torch.optim.Adam step and
DevicePolicy.refresh() (on the same modules, back in eval mode) form a whole update with no copy. There is no Adam kernel for
these buffers. Nothing here synchronises with the host; the outputs are buffers owned by the learner, one set per (N, stream).
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


class _TrainNet:
    """One network's module and its three flat buffers."""

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


class DevicePPOLearner:
    """PPOAgent.update()'s networks, loss and gradients on the device (module docstring). The hyper-parameters default to the
    reference agent's. Dropout is ignored.

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
      advantage gives a FINITE loss over NaN actor gradients (exp's backward, 0 x inf): check the gradients, not the loss alone.
    1 <= N <= 4096; states are float32 (N,16) as RolloutCollector.sample returns them, not packed boards."""

    def __init__(self, actor, critic, clip_epsilon=0.3, value_coef=0.4, entropy_coef=0.05):
        for v, name in ((clip_epsilon, "clip_epsilon"), (value_coef, "value_coef"), (entropy_coef, "entropy_coef")):
            if not (float(v) >= 0.0 and float(v) != float("inf")):
                raise ValueError("%s: %s must be finite and not negative" % (NAME, name))
        self.clip_epsilon, self.value_coef, self.entropy_coef = float(clip_epsilon), float(value_coef), float(entropy_coef)
        self.actor, self.critic = _TrainNet(actor, 4), _TrainNet(critic, 1)
        if self.actor.device != self.critic.device:
            raise ValueError("%s: actor and critic live on different devices" % NAME)
        self.device = self.actor.device
        self._out = OutputCache(NAME, self.device)

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

    def _forward(self, net, states, make):
        n = self._rows(states)
        out = ops.ppo_forward_train(states, net.plain, net.n_out, running=net.running, out=self._out.get(n, make),
                                    workspace=self._out.get(n, _workspace))
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
        n = self._rows(states)
        losses, _, _ = ops.ppo_loss_grad(states, actions, old_log_probs, advantages, returns, self.actor.plain, self.critic.plain,
                                         self.actor.running, self.critic.running, self.clip_epsilon, self.value_coef, self.entropy_coef,
                                         grad_actor=self.actor.grad, grad_critic=self.critic.grad, losses=self._out.get(n, _losses),
                                         workspace=self._out.get(n, _workspace))
        self.actor.tracked(n)
        self.critic.tracked(n)
        return losses
