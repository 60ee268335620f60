"""GPU tests (-m gpu) of the attention kernel's work decompositions: mslam_attention_bf16_cfg runs a forced (key split,
query groups per block) pair.  The query groups of a block only share the K/V ring and the merge buffer: every query row
runs the same floating-point operations in the same order whatever the group count, so for one key split every group
count must give the SAME BITS (torch.equal on the bit patterns, no tolerance), and each pair on its own must stay inside
kernel_refs.attention_bound of the float64 product.  The output lives in a guarded buffer that is refilled before every
launch: a row no block visits keeps the NaN pattern, a row >= nq stored by mistake lands in the next batch element or in
the guard behind O."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = ((1, 2), (2, 2), (2, 4), (4, 2))     # every (split, qg) that csrc/attention.hip instantiates
Q_MAX = 32 * max(qg for _, qg in CONFIGS)                      # query rows of the largest block
STRADDLE_SHAPES = [(2, 2, nq, nk) for nq in (1, 33, Q_MAX - 1, Q_MAX + 1) for nk in (8, 72, 264)]
ENCODER_SHAPE = (12, 16, 768, 768)


def _lib():
    import mslam_hip as m

    return m


def _parent_split(B, H, nq):
    """The key split mslam_attention_bf16 has always used: a function of the number of 64-row blocks."""
    return 4 if -(-nq // 64) * H * B <= 256 else 2


@functools.lru_cache(maxsize=None)
def _case(B, H, nq, nk, kind):
    """Inputs and the float64 statement of one case, computed once for every test that uses it (read-only)."""
    q, k, v = R.attention_inputs(B, H, nq, nk, kind)
    ref, pabs, _ = R.attention_ref(q, k, v)
    return q, k, v, ref, pabs


def _buffers(device, q, k, vt, B, H, nq):
    return {"q": R.Guarded(device, torch.bfloat16, src=q), "k": R.Guarded(device, torch.bfloat16, src=k),
            "vt": R.Guarded(device, torch.bfloat16, src=vt), "o": R.Guarded(device, torch.bfloat16, (B, nq, H * 64))}


def _launch(bufs, shape, split, qg, what):
    """One launch into the refilled O; split None: the default entry point.  Returns O's bit patterns (a copy)."""
    m = _lib()
    B, H, nq, nk = shape
    bufs["o"].refill()
    p = [m.ptr(bufs[n].t) for n in ("q", "k", "vt", "o")]
    if split is None:
        rc = m.lib().mslam_attention_bf16(*p, B, H, nq, nk, m.stream_ptr())
    else:
        rc = m.lib().mslam_attention_bf16_cfg(*p, B, H, nq, nk, split, qg, m.stream_ptr())
    m.check(rc, what)
    R.check_guards(bufs, ["o"], what)
    return bufs["o"].t.view(torch.int16).clone()


@pytest.mark.parametrize("kind", ["leak", "spike"])
@pytest.mark.parametrize("B,H,nq,nk", R.ATTN_SHAPES + STRADDLE_SHAPES)
def test_query_groups_give_the_same_bits(device, B, H, nq, nk, kind):
    """Every instantiated (split, qg) against (split, 2), bit for bit, on kernel_refs.ATTN_SHAPES and on the shapes that
    straddle the largest block (nq = 1, 33, Q_MAX - 1, Q_MAX + 1: waves and whole query groups beyond nq, which still
    take part in every DMA issue and barrier; nk = 8, 72 at split 4: a key tile alone in its split, empty splits)."""
    q, k, v = R.attention_inputs(B, H, nq, nk, kind)
    bufs = _buffers(device, q, k, v.transpose(-1, -2).contiguous(), B, H, nq)
    shape = (B, H, nq, nk)
    base = {}
    for split, qg in sorted(CONFIGS, key=lambda c: (c[0], c[1])):
        out = _launch(bufs, shape, split, qg, f"attention {shape} {kind} split {split} qg {qg}")
        if qg == 2:
            base[split] = out
        else:
            differ = int((out != base[split]).sum())
            assert torch.equal(out, base[split]), f"split {split}: qg {qg} differs from qg 2 in {differ} elements"


@pytest.mark.parametrize("kind", ["leak", "spike"])
@pytest.mark.parametrize("B,H,nq,nk", R.ATTN_SHAPES)
def test_every_config_bounded(device, B, H, nq, nk, kind):
    """|out - float64 softmax(q k^T) v| <= kernel_refs.attention_bound for every instantiated (split, qg), as
    test_kernel_edges_gpu.py::test_attention_bounded asserts for the default path."""
    q, k, v, ref, pabs = _case(B, H, nq, nk, kind)
    bound = R.attention_bound(ref, pabs)
    bufs = _buffers(device, q, k, v.transpose(-1, -2).contiguous(), B, H, nq)
    shape = (B, H, nq, nk)
    for split, qg in CONFIGS:
        what = f"attention {shape} {kind} split {split} qg {qg}"
        out = _launch(bufs, shape, split, qg, what).view(torch.bfloat16).cpu().double()
        err = (out - ref).abs()
        print(f"{what}: max err/bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), f"{what}: err/bound up to {float((err / bound).max())}"


@pytest.mark.parametrize("B,H,nq,nk", [(2, 3, 65, 264), (3, 11, 520, 264)])
def test_default_dispatch_keeps_the_split(device, B, H, nq, nk):
    """mslam_attention_bf16 picks the query groups per shape but the key split as it always has: its output is the bits of
    (that split, 2) on one shape of each split."""
    q, k, v = R.attention_inputs(B, H, nq, nk, "spike")
    bufs = _buffers(device, q, k, v.transpose(-1, -2).contiguous(), B, H, nq)
    shape = (B, H, nq, nk)
    want = _launch(bufs, shape, _parent_split(B, H, nq), 2, f"attention {shape} cfg")
    got = _launch(bufs, shape, None, None, f"attention {shape} default")
    assert torch.equal(got, want), f"{int((got != want).sum())} elements differ"


def test_default_dispatch_encoder_shape(device):
    """The same on the encoder's batch of 12 frames (16 heads, 768 x 768), bits only."""
    B, H, nq, nk = ENCODER_SHAPE
    g = torch.Generator(device=device).manual_seed(12)
    q = (torch.randn(B, H, nq, 64, generator=g, device=device) * 0.125).to(torch.bfloat16)
    k = torch.randn(B, H, nk, 64, generator=g, device=device).to(torch.bfloat16)
    vt = torch.randn(B, H, 64, nk, generator=g, device=device).to(torch.bfloat16)
    bufs = _buffers(device, q, k, vt, B, H, nq)
    assert _parent_split(B, H, nq) == 2
    want = _launch(bufs, ENCODER_SHAPE, 2, 2, "attention encoder cfg")
    got = _launch(bufs, ENCODER_SHAPE, None, None, "attention encoder default")
    assert torch.equal(got, want), f"{int((got != want).sum())} elements differ"


def test_cfg_rejects_what_is_not_instantiated(device):
    """Any other (split, qg) is MSLAM_EINVAL and stores nothing."""
    m = _lib()
    B, H, nq, nk = 1, 2, 33, 72
    q, k, v = R.attention_inputs(B, H, nq, nk, "spike")
    bufs = _buffers(device, q, k, v.transpose(-1, -2).contiguous(), B, H, nq)
    p = [m.ptr(bufs[n].t) for n in ("q", "k", "vt", "o")]
    einval = m.header_constants()["MSLAM_EINVAL"]
    for split in (-2, 0, 1, 2, 3, 4, 8, 18):
        for qg in (-2, 0, 1, 2, 3, 4, 6, 8, 16, 18, 34):
            if (split, qg) not in CONFIGS:
                rc = m.lib().mslam_attention_bf16_cfg(*p, B, H, nq, nk, split, qg, m.stream_ptr())
                assert rc == einval, (split, qg, rc)
    assert bool((bufs["o"].raw == bufs["o"].pat).all()), "a rejected configuration stored to O"
    R.check_guards(bufs, [], "attention cfg rejected")
