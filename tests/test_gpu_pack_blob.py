"""The blobs of ops.tpolicy_pack and ops.qnet_pack on the MI355X, byte for byte against a blob assembled here in NumPy from the
layout documented at the top of csrc/g2048_tpolicy.hip and csrc/g2048_qnet.hip (and csrc/g2048_mfma.h for a fragment). The
forward tests cannot see a padding word; this one sees every byte: the order of the fragments, the k order inside one, bf16
rounding to nearest even, the zero rows past a matrix (the head tile's actor rows over its critic row; the Q-network's four fc
rows), conv2's and the embedding's column permutations, the f32 section and its zero padding.

The smallest legal shape (dim_ff 32, one layer) and dim_ff 96 with three layers (an odd number of 32-feature slices, linear2 with
three bf16 chunks, the second and third layers' offsets l * layer_frags() and l * layer_params()), assembled by one function of
(dim_ff, layers) on the hash weights of tests/tpolicy_weights.py / tests/qnet_weights.py, whose values
have 16 significant bits, so bf16 rounding is exercised, ties included. The bf16 reference rounds with torch's own float32 ->
bfloat16 conversion, not with the kernel's integer formula."""
import numpy as np
import pytest
import torch

import qnet_weights as qw
import tpolicy_weights as tw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
# the smallest legal shape, and three 32-feature slices (an odd chunk count of linear2 in bf16, a fragment index o * c2 + c with c2
# no power of two) with a third layer's offset in the fragments and in the f32 section
SHAPES = [(32, 1), (96, 3)]


def bf16_bits(x):
    """float32 array -> its bfloat16 bit patterns (uint32 array), rounded as torch rounds"""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().astype(np.uint16).astype(np.uint32).reshape(x.shape)


def fragments(w, bf16):
    """A matrix [rows][K] (float32, columns already in packed k order) as packed words, fragments ordered [row tile][chunk]:
    lane l of a fragment holds row 16 o + (l & 15); with g = l >> 4, f32 word r is k = 16 c + 4 g + r, bf16 element j is
    k = 32 c + 16 (j >> 2) + 4 g + (j & 3), two elements a word, the even one in the low half. Rows past the matrix are zero."""
    rows, K = w.shape
    tiles = (rows + 15) // 16
    full = np.zeros((16 * tiles, K), np.float32)
    full[:rows] = w
    chunk = 32 if bf16 else 16
    o, c, lane = np.meshgrid(np.arange(tiles), np.arange(K // chunk), np.arange(64), indexing="ij")
    row, g = 16 * o + (lane & 15), lane >> 4
    if not bf16:
        k = (16 * c + 4 * g)[..., None] + np.arange(4)
        return full[row[..., None], k].view(np.uint32).reshape(-1)
    j = np.arange(8)
    k = (32 * c + 4 * g)[..., None] + 16 * (j >> 2) + (j & 3)
    e = bf16_bits(full[row[..., None], k])
    return (e[..., 0::2] | (e[..., 1::2] << 16)).astype(np.uint32).reshape(-1)


def floats(*parts):
    return np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in parts]).view(np.uint32)


def plain_buffer(sd, shapes):
    """The plain parameter buffer of include/g2048.h: state-dict order, the two LayerNorm eps after each layer's norm2.bias."""
    out = []
    for name, _ in shapes:
        out.append(sd[name].astype(np.float32).reshape(-1))
        if name.endswith("norm2.bias"):
            out.append(np.array([EPS, EPS], np.float32))
    return np.concatenate(out)


def tpolicy_case(bf16, dim_ff, layers):
    shapes = tw.reference_shapes(dim_ff, layers)
    sd = {k: v.astype(np.float32) for k, v in tw.state_dict(shapes).items()}
    mats, params = [], [sd["embedding.weight"], sd["embedding.bias"]]
    for l in range(layers):
        p = "transformer_encoder.layers.%d." % l
        mats += [sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.out_proj.weight"], sd[p + "linear1.weight"], sd[p + "linear2.weight"]]
        params += [sd[p + "self_attn.in_proj_bias"], sd[p + "self_attn.out_proj.bias"], sd[p + "linear1.bias"], sd[p + "linear2.bias"],
                   sd[p + "norm1.weight"], sd[p + "norm1.bias"], sd[p + "norm2.weight"], sd[p + "norm2.bias"], [EPS, EPS, 0.0, 0.0]]
    mats += [sd["fc1.weight"], sd["fc2.weight"], np.concatenate([sd["actor.weight"], sd["critic.weight"]])]
    head_bias = np.zeros(16, np.float32)
    head_bias[:4], head_bias[4] = sd["actor.bias"], sd["critic.bias"][0]
    params += [sd["fc1.bias"], sd["fc2.bias"], head_bias]
    return plain_buffer(sd, shapes), np.concatenate([fragments(m, bf16) for m in mats] + [floats(*params)])


def qnet_case(bf16, dim_ff, layers):
    shapes = qw.reference_shapes(dim_ff, layers)
    sd = {k: v.astype(np.float32) for k, v in qw.state_dict(shapes).items()}
    conv2 = sd["cnn.2.weight"].reshape(64, 32, 4).transpose(0, 2, 1).reshape(64, 128)             # k = tap * 32 + channel
    emb = sd["embedding.weight"].reshape(128, 64, 16).transpose(0, 2, 1).reshape(128, 1024)      # k = position * 64 + channel
    mats = [conv2, emb]
    params = [sd["cnn.0.weight"].reshape(32, 4).T, sd["cnn.0.bias"], sd["cnn.2.bias"], sd["embedding.bias"]]     # conv1 [tap][channel]
    for l in range(layers):
        p = "transformer.layers.%d." % l
        mats += [sd[p + "self_attn.in_proj_weight"][256:], sd[p + "self_attn.out_proj.weight"], sd[p + "linear1.weight"], sd[p + "linear2.weight"]]
        params += [sd[p + "self_attn.in_proj_bias"][256:], sd[p + "self_attn.out_proj.bias"], sd[p + "linear1.bias"], sd[p + "linear2.bias"],
                   sd[p + "norm1.weight"], sd[p + "norm1.bias"], sd[p + "norm2.weight"], sd[p + "norm2.bias"], [EPS, EPS, 0.0, 0.0]]
    mats.append(sd["fc.weight"])
    fc_bias = np.zeros(16, np.float32)
    fc_bias[:4] = sd["fc.bias"]
    params.append(fc_bias)
    return plain_buffer(sd, shapes), np.concatenate([fragments(m, bf16) for m in mats] + [floats(*params)])


CASES = [(net, precision, shape) for shape in SHAPES for precision in ("f32", "bf16") for net in ("tpolicy", "qnet")]


@pytest.mark.parametrize("net,precision,shape", CASES, ids=["%s-%s" % c[:2] + ("" if c[2] == SHAPES[0] else "-ff%d-L%d" % c[2]) for c in CASES])
def test_packed_blob_is_the_documented_layout_byte_for_byte(net, precision, shape):
    from g2048 import ops
    dim_ff, layers = shape
    plain, want = (tpolicy_case if net == "tpolicy" else qnet_case)(precision == "bf16", dim_ff, layers)
    pack, size = (ops.tpolicy_pack, ops.tpolicy_packed_bytes) if net == "tpolicy" else (ops.qnet_pack, ops.qnet_packed_bytes)
    assert want.nbytes == size(precision, dim_ff, layers)
    out = torch.full((want.nbytes,), 0xA5, dtype=torch.uint8, device=DEV)           # every byte must be written
    got = pack(torch.from_numpy(plain).to(DEV), dim_ff, layers, precision, out=out).cpu().numpy().view(np.uint32)
    wrong = np.flatnonzero(got != want)
    print("%s %s dim_ff %d L %d: %d bytes, %d of %d words differ%s" % (net, precision, dim_ff, layers, want.nbytes, len(wrong), len(want),
                                                                       "" if not len(wrong) else ", the first at word %d" % wrong[0]))
    assert len(wrong) == 0
