"""What the CPU and the GPU tests of the Q-network's loss and gradient pass share: the inputs' recipe, the stock module's own
autograd through the lines of train_step (the yardstick in float64, the tolerance's measure in float32), and the plain layout's
offsets, and layer 0's attention probabilities from the float64 module. Tensors are numbered in the plain layout's order, which is the module's parameter order."""
import numpy as np
import torch
import torch.nn as nn

N_UPSTREAM = 8          # cnn.*, embedding.*, layer 0's in_proj_*: the parameters upstream of layer 0's softmax, first in the layout
F32_FACTOR = 8.0


def recipe(n):
    """(actions int64, target offsets float64, weights float32) of row i: every action present, both Huber branches populated."""
    i = np.arange(n, dtype=np.int64)
    return (5 * i + 1) % 4, ((37 * i + 11) % 101 - 50) / 25.0, (0.25 + ((13 * i) % 16) / 16.0).astype(np.float32)


def tile_values(codes, dtype):
    b = np.asarray(codes)
    return torch.from_numpy(np.where(b > 0, 2.0 ** b.astype(np.float64), 0.0)).to(dtype)


def case_inputs(model64, codes):
    """(actions, targets float32, weights) by the recipe, the targets around the float64 module's own Q."""
    n = len(codes)
    a, offset, w = recipe(n)
    with torch.no_grad():
        q = model64(tile_values(codes, torch.float64)).numpy()
    return a, (q[np.arange(n), a] + offset).astype(np.float32), w


def stock_loss_grad(model, codes, actions, targets, weights):
    """hybrid.py:1038, :1049-1055 on the stock module in its own dtype: (loss, td, q, [gradient per parameter]) as float64 NumPy."""
    dtype = next(model.parameters()).dtype
    q = model(tile_values(codes, dtype))
    td = nn.SmoothL1Loss(reduction="none")(q.gather(1, torch.from_numpy(actions).unsqueeze(1)).squeeze(1), torch.from_numpy(targets).to(dtype))
    loss = (torch.from_numpy(weights).to(dtype) * td).mean()
    model.zero_grad()
    loss.backward()
    grads = [p.grad.detach().numpy().astype(np.float64).reshape(-1) for p in model.parameters()]
    model.zero_grad()
    return float(loss.detach()), td.detach().numpy().astype(np.float64), q.detach().numpy().astype(np.float64), grads


def layer0_attention(model64, codes):
    """(logits, P) of layer 0's attention from the float64 module alone, both [head][query][key]: the boards of the call are one
    sequence, P is the softmax over the keys of q . k / sqrt(16) per head, q and k from embedding(cnn(x)) through in_proj."""
    n = len(codes)
    attn = model64.transformer.layers[0].self_attn
    with torch.no_grad():
        h = model64.embedding(model64.cnn(tile_values(codes, torch.float64).view(-1, 1, 4, 4)).view(n, -1))
        qk = h @ attn.in_proj_weight[:256].T + attn.in_proj_bias[:256]
        q, k = qk[:, :128].view(n, 8, 16), qk[:, 128:].view(n, 8, 16)
        logits = torch.einsum("ihd,jhd->hij", q, k) / 4.0
        return logits.numpy(), torch.softmax(logits, -1).numpy()


def plain_slices(parsed):
    """([(offset, numel) per tensor], [offsets of the LayerNorm-eps slots], total) of the parsed module's plain layout."""
    slices, eps, o = [], [], 0
    for t in parsed.plain_tensors():
        if isinstance(t, torch.Tensor):
            slices.append((o, t.numel()))
            o += t.numel()
        else:
            eps.append(o)
            o += 1
    return slices, eps, o


def ratios(got, want):
    """max|got - want| / max|want| per tensor; a tensor whose gradient is exactly zero (conv1.weight on an empty board) must be
    exactly zero: 0 then, inf otherwise."""
    out = []
    for g, w in zip(got, want):
        err, top = np.abs(np.asarray(g, np.float64) - w).max(), np.abs(w).max()
        out.append(err / top if top > 0 else (0.0 if err == 0 else np.inf))
    return np.array(out)
