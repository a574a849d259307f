"""What tests/qnet_dropout_ref.py and tests/tpolicy_dropout_ref.py share: the mask rule of an encoder network's training-mode
dropout and the stock module fed those masks, once, for a network described by an Encoder.

The mask rule, restated in NumPy uint32 from its specification (include/g2048_train.h, include/g2048_ttrain.h), not imported from
the library: for the library call with index c, (k0, k1) = rng_keys(seed, the network's domain, c); element e of site s of encoder
layer L draws h = rng_draw(k0, k1, ((4 L + s) << 32) | e, 0) and is kept iff h >= T = floor(p_s 2^32); a kept element is multiplied
by 1 / (1 - p_s), a dropped one by 0. The hash itself (splitmix64, rng_keys, rng_draw) is the restatement tests/ppo_dropout_ref.py
already holds.

The yardstick: the STOCK module in .train() mode, fed those masks by replacing torch.nn.functional.dropout and
torch.nn.functional.scaled_dot_product_attention for the duration of a call (feeding()). The training-mode layer calls them in the
order SDPA, dropout1, the hidden layer's dropout, dropout2 per layer, which is the order of the sites; every call asserts its shape
(the Encoder's q_shape and dropout_shape) and the probability torch passes.
"""
import contextlib
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

from ppo_dropout_ref import rng_draws, rng_keys, scale32, scale64, threshold


@functools.lru_cache(maxsize=512)
def _whole_mask(enc, seed, call_index, layer, site, p, n, dim_ff):
    return enc.keep_mask(seed, call_index, layer, site, p, n, dim_ff)


class Encoder:
    """One network: its RNG domain, site_shape(site, n, dim_ff) -> (rows, columns) of a site's matrix, q_shape(n): the shape of
    the q that scaled_dot_product_attention is called with, dropout_shape(n, width): of the input of a dropout call over `width`
    features, layers(model): the module's encoder layers."""

    def __init__(self, domain, site_shape, q_shape, dropout_shape, layers):
        self.domain, self.site_shape, self.q_shape, self.dropout_shape, self.layers = domain, site_shape, q_shape, dropout_shape, layers
        self.width = site_shape(1, 1, 0)[1]          # d_model

    def keep_mask(self, seed, call_index, layer, site, p, n, dim_ff, rows=None):
        """bool (rows, columns): which elements of rows [first, first + count) (rows = (first, count); None: all) of site `site` of
        encoder layer `layer` the call keeps."""
        height, width = self.site_shape(site, n, dim_ff)
        first, count = (0, height) if rows is None else rows
        assert 0 <= first and first + count <= height
        k0, k1 = rng_keys(seed, self.domain, call_index)
        e = np.arange(first * width, (first + count) * width, dtype=np.uint64).astype(np.uint32)
        return (rng_draws(k0, k1, 4 * layer + site, e) >= np.uint32(threshold(p))).reshape(count, width)

    def multiplier(self, seed, call_index, layer, site, p, n, dim_ff, dtype):
        """keep x scale as a tensor in dtype: the double scale in float64, the project's float32(1 / (1 - p)) in float32."""
        scale = scale64(p) if dtype == torch.float64 else float(scale32(p))
        return torch.from_numpy(_whole_mask(self, seed, call_index, layer, site, float(p), n, dim_ff)).to(dtype) * scale

    @contextlib.contextmanager
    def feeding(self, seed, call_index, p4, n, dim_ff):
        """While it is open, the training-mode encoder layers draw no random numbers: scaled_dot_product_attention is
        softmax(q k^T / 4) x the site-0 multipliers, then . v, and dropout is input x the site's multipliers, the sites told by the
        order of the calls. Yields the call counter (a list of one int)."""
        calls = [0]
        real_dropout, real_sdpa = F.dropout, F.scaled_dot_product_attention

        def mult(site, shape, dtype):
            layer, s = divmod(calls[0], 4)
            assert s == site, "call %d of the layer is site %d, expected %d" % (calls[0], s, site)
            calls[0] += 1
            return self.multiplier(seed, call_index, layer, site, p4[site], n, dim_ff, dtype).reshape(shape)

        def sdpa(q, k, v, attn_mask=None, dropout_p=0.0, is_causal=False, **kw):
            assert tuple(q.shape) == self.q_shape(n) and attn_mask is None and not is_causal and dropout_p == p4[0], (q.shape, dropout_p)
            prob = torch.softmax(q @ k.transpose(-1, -2) / 4.0, dim=-1)
            return (prob * mult(0, prob.shape, q.dtype)) @ v

        def dropout(x, p=0.5, training=True, inplace=False):
            site = calls[0] % 4
            assert site != 0 and training and p == p4[site] and tuple(x.shape) == self.dropout_shape(n, dim_ff if site == 2 else self.width), (
                site, p, x.shape)
            return x * mult(site, x.shape, x.dtype)

        F.dropout, F.scaled_dot_product_attention = dropout, sdpa
        try:
            yield calls
        finally:
            F.dropout, F.scaled_dot_product_attention = real_dropout, real_sdpa

    def training_copy(self, model, p4, dtype):
        """A deep copy of the module in dtype and .train() mode whose layers carry the four probabilities."""
        m = copy.deepcopy(model).to(dtype).train()
        for lay in self.layers(m):
            lay.self_attn.dropout, lay.dropout1.p, lay.dropout.p, lay.dropout2.p = p4
        return m

    def dims(self, model):
        return self.layers(model)[0].linear1.out_features, len(self.layers(model))
