"""The gate of tests/test_gpu_conv_grade.py tested on the CPU, against a torch emulation of the backbone kernels' precision contract
(tests/conv_cases.py): on every convolution, weight-gradient and data-gradient case of the GPU file the unbroken emulation passes the
gate - so the gate is reachable by the contract alone, measured against the fp32 CPU operators and not against a kernel - and each single
defect (a lost cross term on the whole tensor, on one output channel of 512, one tap of nine, one image of three, one halo column, one
pixel; a lost lo plane; one scale per tensor where the contract has one per 32 pixels) fails it - the lost term on one channel of a
512-channel weight gradient and a wrong channel of dgamma / dbeta while the whole-tensor rel_err stays below the older tests' 1e-5.
Masks and pool winners of every case agree between the fp32 and fp64 references with a margin, and the span of a batch the per-tensor scale can carry is measured: 100 x per image in, 1000 x out."""

import pytest
import torch

import conv_cases as cc
import parity
from conftest import rel_err

CONV = cc.conv3x3_cases() + cc.conv1x1_cases() + cc.conv_s2_cases()
N_CAP = 3   # images per case here (the 8- and 9-image cases exist for the GPU grid's tile count: the arithmetic of an image is the same)


def _cap(kw):
    return dict(kw, N=min(kw["N"], N_CAP))


def _no_factor_8(cid, pairs):
    """A case outside conv_cases.WIDE keeps the default gate because the contract alone needs at most half of it (the issue's rule for factor 8)."""
    if cid not in cc.WIDE:
        t = cc.tightness(pairs)
        assert t <= 0.5, (cid, t)


@pytest.mark.parametrize("cid,kw", CONV, ids=[c for c, _ in CONV])
def test_conv_gate_passes_the_contract_and_fails_a_lost_term(cid, kw):
    c = cc.conv_case(**_cap(kw))
    cc.grade(cc.emulated_conv_case(c), c.want64, c.want32, c.label + " emulated", **cc.gate_of("conv-" + cid))
    _no_factor_8("conv-" + cid, cc.act_pairs(cc.emulated_conv_case(c), c.want64, c.want32))
    for drop in ("lo.hi", "hi.lo"):
        with pytest.raises(AssertionError):
            cc.grade(cc.emulated_conv_case(c, drop=drop), c.want64, c.want32, f"{c.label} without {drop}", **cc.gate_of("conv-" + cid))


@pytest.mark.parametrize("cid,kw", cc.stem_cases(), ids=[c for c, _ in cc.stem_cases()])
def test_stem_gate_passes_the_contract_and_fails_a_lost_term(cid, kw):
    c = cc.stem_case(**kw)
    cc.grade(cc.emulated_stem_case(c), c.want64, c.want32, c.label + " emulated", **cc.gate_of("stem-" + cid))
    _no_factor_8("stem-" + cid, cc.act_pairs(cc.emulated_stem_case(c), c.want64, c.want32))
    for drop in ("lo.hi", "hi.lo"):
        with pytest.raises(AssertionError):
            cc.grade(cc.emulated_stem_case(c, drop=drop), c.want64, c.want32, f"{c.label} without {drop}", **cc.gate_of("stem-" + cid))


STRIP, WAVE, STEMW = cc.wgrad_strip_cases(), cc.wgrad_wave_cases(), cc.stem_wgrad_cases()


def _emulated_dw(c, words, **kw):
    if words:
        return cc.emulated_wgrad(c.dy, c.x, c.wshape, c.stride, **kw)
    return cc.emulated_wgrad_blocks(c.dy, c.x, c.wshape, c.stride, **kw)


def _wgrad_all():
    out = [("strip-" + cid, kw, True, cc.wgrad_case) for cid, kw in STRIP]
    out += [("wave-" + cid, kw, words, cc.wgrad_case) for cid, kw, words in WAVE]
    out += [("stemw-" + cid, kw, True, cc.stem_wgrad_case) for cid, kw in STEMW]
    return out


@pytest.mark.parametrize("cid,kw,words,build", _wgrad_all(), ids=[c[0] for c in _wgrad_all()])
def test_wgrad_gate_passes_the_contract_and_fails_a_lost_term(cid, kw, words, build):
    c = build(**kw)
    gate = cc.gate_of(cid)
    cc.grade_dw(_emulated_dw(c, words), c.want64, c.want32, c.label + " emulated", row_self=c.row_self, **gate)
    _no_factor_8(cid, cc.dw_pairs(_emulated_dw(c, words), c.want64, c.want32))
    for drop in ("lo.hi", "hi.lo"):   # = the lost lo plane of dY, of X
        with pytest.raises(AssertionError):
            cc.grade_dw(_emulated_dw(c, words, drop=drop), c.want64, c.want32, f"{c.label} without {drop}", row_self=c.row_self, **gate)


@pytest.mark.parametrize("cid,kw", cc.dgrad_cases(), ids=[c for c, _ in cc.dgrad_cases()])
def test_dgrad_gate_passes_the_contract_and_fails_a_lost_term(cid, kw):
    c = cc.dgrad_case(**kw)
    gate = cc.gate_of("dgrad-" + cid)
    cc.grade(cc.emulated_dgrad_case(c), c.want64, c.want32, c.label + " emulated", **gate)
    _no_factor_8("dgrad-" + cid, cc.act_pairs(cc.emulated_dgrad_case(c), c.want64, c.want32))
    for drop in ("lo.hi", "hi.lo"):
        with pytest.raises(AssertionError):
            cc.grade(cc.emulated_dgrad_case(c, drop=drop), c.want64, c.want32, f"{c.label} without {drop}", **gate)


def test_widened_gates_are_the_justified_ones():
    """Every entry of conv_cases.WIDE names a case of the GPU file; factor 8 only where the unbroken emulation exceeds half the default bound,
    the 2^-20 floor only on contractions of fewer than 64 terms, where the emulation passes it at or below one half; the recorded ratio is
    the one measured here."""
    known = {}
    for cid, kw in CONV:
        known["conv-" + cid] = ("conv", kw)
    for cid, kw in cc.stem_cases():
        known["stem-" + cid] = ("stem", kw)
    for cid, kw, words, build in _wgrad_all():
        known[cid] = ("dw", (kw, words, build))
    for cid, kw in cc.dgrad_cases():
        known["dgrad-" + cid] = ("dgrad", kw)
    assert set(cc.WIDE) <= set(known)
    for cid, (factor, floor, recorded) in cc.WIDE.items():
        what, kw = known[cid]
        if what == "dw":
            c = kw[2](**kw[0])
            pairs = cc.dw_pairs(_emulated_dw(c, kw[1]), c.want64, c.want32)
        elif what == "conv":
            c = cc.conv_case(**_cap(kw))
            pairs = cc.act_pairs(cc.emulated_conv_case(c), c.want64, c.want32)
        elif what == "stem":
            c = cc.stem_case(**kw)
            pairs = cc.act_pairs(cc.emulated_stem_case(c), c.want64, c.want32)
        else:
            c = cc.dgrad_case(**kw)
            pairs = cc.act_pairs(cc.emulated_dgrad_case(c), c.want64, c.want32)
        t = cc.tightness(pairs)
        print(f"{cid:48s} emulation / default bound {t:5.2f} (recorded {recorded:5.2f})  gate {factor:g} x + {floor:.2e}")
        assert abs(t - recorded) <= 0.02 + 0.02 * recorded, (cid, t, recorded)
        assert (factor, floor) in ((8.0, parity.FLOOR), (parity.FACTOR, cc.FLOOR_SHORT), (8.0, cc.FLOOR_SHORT)), cid
        if factor == 8.0:
            assert t > 0.5, (cid, t)
        if floor == cc.FLOOR_SHORT:
            assert what == "dw" and c.terms < cc.SHORT_TERMS, cid
            assert cc.tightness(pairs, parity.FACTOR, cc.FLOOR_SHORT) <= 0.5, cid


# ---- confined defects: the gate sees them, the whole-tensor norm at the older bar does not -----------------------------------------------
OLD_TRAIN_BAR = 1e-5   # test_gpu_conv_training.py: weight gradients, dgamma, dbeta


@pytest.mark.parametrize("where", [{"channel": 300}, {"tap": (0, 2)}, {"image": 1}, {"column": 0}, {"pixel": (2, 4, 3)}],
                         ids=["one-channel-of-512", "one-tap-of-nine", "one-image-of-three", "one-halo-column", "one-pixel"])
def test_a_confined_lost_term_fails_the_weight_gradient_gate_below_the_old_bar(where):
    c = cc.wgrad_case(512, 512, 3, 9, 5, seed=41)
    cc.grade_dw(cc.emulated_wgrad(c.dy, c.x, c.wshape), c.want64, c.want32, c.label + " emulated")
    for drop in ("lo.hi", "hi.lo"):
        bad = cc.emulated_wgrad(c.dy, c.x, c.wshape, drop=drop, where=where)
        e = rel_err(bad, c.want64)
        print(f"{c.label} without {drop} at {where}: whole-tensor rel_err {e:.2e}")
        if "channel" in where:   # (a tap, an image, a column or one pixel of 135 moves the norm above the old bar as well)
            assert e < OLD_TRAIN_BAR, e
        with pytest.raises(AssertionError):
            cc.grade_dw(bad, c.want64, c.want32, f"{c.label} without {drop} at {where}")


@pytest.mark.parametrize("where", [{"channel": 300}, {"tap": (0, 2)}, {"image": 1}, {"column": 0}, {"pixel": (2, 4, 3)}],
                         ids=["one-channel-of-512", "one-tap-of-nine", "one-image-of-three", "one-halo-column", "one-pixel"])
def test_a_confined_lost_term_fails_the_convolution_gate(where):
    """Every confined defect fails the gate on the inference side as well (where the older bar, 2e-6 and 8 * e32 + 2e-7 on the norm, is tight
    enough to catch them too: the figures are printed)."""
    c = cc.conv_case(512, 512, 3, 9, 17, relu=False, fold=False, seed=42)
    cc.grade(cc.emulated_conv_case(c), c.want64, c.want32, c.label + " emulated")
    bad = cc.emulated_conv_case(c, drop="lo.hi", where=where)
    e, e32 = rel_err(bad, c.want64), rel_err(c.want32, c.want64)
    print(f"{c.label} without lo.hi at {where}: whole-tensor rel_err {e:.2e} (fp32 {e32:.2e})")
    with pytest.raises(AssertionError):
        cc.grade(bad, c.want64, c.want32, f"{c.label} without lo.hi at {where}")


def test_a_wrong_channel_of_a_channel_vector_fails_the_gate_below_the_old_bar():
    """dgamma / dbeta of 512 channels with ONE typical channel off by 1e-4 of itself (what a lost term costs): 4e-6 on the norm, under the 1e-5 bar."""
    c = cc.bn_case(512, 129, relu=True, res=False, seed=43)
    cc.grade_vec(c.b32.vec, c.b64.vec, c.b32.vec, c.label + " fp32 itself")
    for name in ("dgamma", "dbeta"):
        bad = {k: v.clone() for k, v in c.b32.vec.items()}
        v = c.b64.vec[name].abs()
        ch = int((v - v.square().mean().sqrt()).abs().argmin())   # a channel of typical size
        bad[name][ch] *= 1.0 + 1e-4
        e = rel_err(bad[name], c.b64.vec[name])
        print(f"{c.label} {name}[{ch}] off by 1e-4: whole-vector rel_err {e:.2e}")
        assert e < OLD_TRAIN_BAR
        with pytest.raises(AssertionError):
            cc.grade_vec(bad, c.b64.vec, c.b32.vec, f"{c.label} {name}[{ch}] off by 1e-4")


def test_one_scale_per_tensor_fails_where_the_contract_has_one_per_32_pixels():
    """The per-wave weight gradient without abs-max words on images 1000 x apart: a scale per 32 pixels of a row carries any span between
    images; one scale per operand (the defect) loses the quiet image's low bits."""
    c = cc.wgrad_case(128, 64, 3, 8, 8, k=1, kind="spread", spread=1000.0, seed=44)
    cc.grade_dw(cc.emulated_wgrad_blocks(c.dy, c.x, c.wshape), c.want64, c.want32, c.label + " emulated, per 32 pixels")
    with pytest.raises(AssertionError):
        cc.grade_dw(cc.emulated_wgrad_blocks(c.dy, c.x, c.wshape, block="tensor"), c.want64, c.want32, c.label + " one scale per tensor")


def test_a_nan_fails_the_gate():
    c = cc.conv_case(64, 64, 2, 3, 5, seed=3)
    got = c.want32.clone()
    cc.grade(got, c.want64, c.want32, "the fp32 path against itself")
    got[1, 7, 2, 3] = float("nan")
    with pytest.raises(AssertionError):
        cc.grade(got, c.want64, c.want32, "one NaN")
    w = cc.wgrad_case(64, 64, 1, 3, 5, seed=4)
    dw = w.want32.clone()
    cc.grade_dw(dw, w.want64, w.want32, "the fp32 weight gradient against itself")
    dw[5, 6, 1, 1] = float("nan")
    with pytest.raises(AssertionError):
        cc.grade_dw(dw, w.want64, w.want32, "one NaN in a weight gradient")
    b = cc.bn_case(64, 5, seed=5)
    vec = {k: v.clone() for k, v in b.b32.vec.items()}
    vec["dbeta"][9] = float("nan")
    with pytest.raises(AssertionError):
        cc.grade_vec(vec, b.b64.vec, b.b32.vec, "one NaN in dbeta")


# ---- nothing left to luck ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,kw", cc.bn_cases(), ids=[c for c, _ in cc.bn_cases()])
def test_no_relu_mask_bit_is_left_to_luck(cid, kw):
    c = cc.bn_case(**kw)
    if c.relu:
        assert torch.equal(c.f32.pre > 0, c.f64.pre > 0)          # every mask bit, no element left out
        assert cc.decision_margin(c) > cc.MASK_MARGIN, cc.decision_margin(c)
        # the recomputed-mask form evaluates bn_affine on the fp32 mean / rstd: the same bits
        if c.res is None:
            again = cc.bn_affine(c.y, c.f32.vec["mean"], c.f32.vec["rstd"], c.gamma, c.beta)
            assert torch.equal(again > 0, c.mask)


@pytest.mark.parametrize("cid,kw", cc.pool_cases(), ids=[c for c, _ in cc.pool_cases()])
def test_no_pool_winner_is_left_to_luck(cid, kw):
    c = cc.pool_case(**kw)
    assert torch.equal(c.f32.idx, c.f64.idx)
    assert cc.decision_margin(c) > cc.MASK_MARGIN, cc.decision_margin(c)
    # the restated first-maximum rule is ATen's: values and the gradient's route agree with max_pool2d(relu(.)) under autograd
    v = c.f64.v.clone().requires_grad_()
    p = torch.nn.functional.max_pool2d(torch.relu(v), 3, 2, 1)
    assert torch.equal(p.detach(), c.f64.p)
    p.backward(c.dp.double())
    mean, rstd = c.f32.vec["mean"].double(), c.f32.vec["rstd"].double()
    xh = (c.y.double() - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)
    assert torch.allclose(c.b64.vec["dbeta"], v.grad.sum(dim=(0, 2, 3)), rtol=1e-12, atol=1e-12)
    assert torch.allclose(c.b64.vec["dgamma"], (v.grad * xh).sum(dim=(0, 2, 3)), rtol=1e-12, atol=1e-12)
    w = cc.winner_words(c.f32.idx)
    assert w.shape == (c.N, c.f32.idx.shape[2], c.f32.idx.shape[3], c.C // 4) and int((w & 255).max()) <= 9


# ---- the span of a batch the per-tensor scale carries ------------------------------------------------------------------------------------
def test_spread_of_100_per_image_passes_and_1000_fails_on_the_image_figure():
    """One scale per tensor: fp16 is a floating-point format, so a value 2^-k below the tensor's largest keeps hi + lo's 22 bits down to
    k = 17 (1.3e5).  Three images 100 x apart put the quiet image 1e4 below the loud one: inside.  1000 x apart: 1e6 - the quiet image
    loses lo's low bits, which the per-image figure shows and the whole-tensor figure does not.  DESIGN.md section 3 states the range from
    these two figures."""
    kw = dict(Cin=128, Cout=128, N=3, H=7, W=15, relu=True, kind="spread", seed=150)
    inside = cc.conv_case(**kw)
    got = cc.emulated_conv_case(inside)
    cc.grade(got, inside.want64, inside.want32, inside.label + " emulated")
    (e, e32), _ = cc.act_pairs(got, inside.want64, inside.want32)
    print(f"100 x per image: worst image {e.traj:.2e} = {e.traj / e32.traj:.2f} x fp32, worst pixel {e.row / e32.row:.2f} x")
    assert e.traj < 2.5 * e32.traj and e.row < 2.5 * e32.row
    outside = cc.conv_case(**dict(kw, spread=1000.0))
    got = cc.emulated_conv_case(outside)
    (e, e32), _ = cc.act_pairs(got, outside.want64, outside.want32)
    print(f"1000 x per image: worst image {e.traj:.2e} = {e.traj / e32.traj:.1f} x fp32, whole tensor {e.glob:.2e} = {e.glob / e32.glob:.2f} x")
    assert e.glob <= parity.FACTOR * e32.glob + parity.FLOOR         # the norm does not see it
    assert e.traj > 10 * e32.traj                                     # the image figure does
    with pytest.raises(AssertionError):
        cc.grade(got, outside.want64, outside.want32, outside.label + " emulated")
    # the weight gradient: x times c_n, dy by 1 / c_n - every image weighs the same, the quiet operands lose their bits
    w = cc.wgrad_case(128, 64, 3, 9, 33, kind="spread", seed=542)
    cc.grade_dw(cc.emulated_wgrad(w.dy, w.x, w.wshape), w.want64, w.want32, w.label + " emulated")
    w = cc.wgrad_case(128, 64, 3, 9, 33, kind="spread", spread=1000.0, seed=542)
    with pytest.raises(AssertionError):
        cc.grade_dw(cc.emulated_wgrad(w.dy, w.x, w.wshape), w.want64, w.want32, w.label + " emulated")


def test_scale_and_split_follow_the_kernels_rule():
    amax = torch.tensor([0.0, 1.0, 0.75, 8192.0, 16383.0, 16384.0, 3e-5, 1e30, 2.0 ** -113, 2.0 ** -114, 1e-40, float("inf")])
    s = cc.scale_of(amax)
    assert s[0] == 1.0 and s[9] == 1.0 and s[10] == 1.0 and s[11] == 1.0     # zero, below 2^-113, subnormal, non-finite
    prod = (amax * s)[1:9]
    assert ((prod >= 8192) & (prod < 16384)).all()
    assert (torch.frexp(s)[0] == 0.5).all()
    x = torch.randn(4000) * 3.0
    sx = cc.scale_of(x.abs().max())
    xs = x.double() * float(sx)
    for rtz in (False, True):
        hi, lo = cc.split(x, sx, rtz=rtz)
        assert float(((hi + lo) - xs).abs().max()) <= 2.0 ** -22 * 16384 * (2 if rtz else 1)
        if rtz:
            assert (hi.abs() <= xs.abs()).all() and ((hi + lo).abs() <= xs.abs()).all()
    hi, lo = cc.split(torch.tensor([2.0 ** -3 + 2.0 ** -26]), 1.0)              # lo below fp16's subnormal quantum 2^-24 is lost
    assert float(lo) == 0.0
    # the emulations are the operators when nothing is dropped, to the contract's precision
    c = cc.conv_case(64, 64, 2, 5, 6, k=3, stride=2, fold=False, seed=9)
    assert rel_err(cc.emulated_conv(c.x, c.w, 2), c.want64) < 1e-6
    w = cc.wgrad_case(64, 64, 2, 5, 6, k=3, stride=2, seed=9)
    assert rel_err(cc.emulated_wgrad(w.dy, w.x, w.wshape, 2), w.want64) < 1e-6
    assert rel_err(cc.emulated_wgrad_blocks(w.dy, w.x, w.wshape, 2), w.want64) < 1e-6
    d = cc.dgrad_case(64, 128, 2, 5, 6, k=3, stride=2, seed=9)
    assert rel_err(cc.emulated_dgrad_case(d), d.want64) < 1e-6
    assert rel_err(cc.emulated_wgrad(w.dy, w.x, w.wshape, 2, drop="lo.hi"), w.want64) > 1e-5
