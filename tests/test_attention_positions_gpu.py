"""GPU: position-resolved checks of the four attention kernel families -- every key of every row is checked, at a RELATIVE
tolerance (mass) or bit for bit (needle).  The inputs, references and comparator are in _attn_positions.py (CPU-tested by
test_attention_positions.py); the randn / absolute-tolerance tests of each family stay where they are.

MASS: value rows are one-hot in the key's position, so o[.., c] is the softmax mass of the keys at positions = c (mod Dv); the
reference is the float64 softmax; |o - p| <= tol_rel * p + 1e-9 per element and EXACTLY 0.0 where no visible key maps (masked
scores are -inf before the exponential in every kernel, nothing else is correct).  tol_rel = (roundings to the 16-bit type between
score and output) x half an ulp (2^-8 bf16, 2^-11 f16) + 2^-12 for the f32 effects (exp2 approximation, the rounded
sm_scale * log2 e).  Every form below has TWO roundings -- P to the value dtype, the output once -- and sums l from the unrounded
f32 exponentials, so tol_rel = 2^-7 + 2^-12 (bf16) and 2^-10 + 2^-12 (f16):

  form                               P rounded                                 l (unrounded terms)   output rounded
  MLA decode   (stage 1 + stage 2)   mla_decode_attention.hip:211              :210, :214            decode_attention.hip:559 (stage 2; the
                                                                                                      partials :232-239 are f32)
  MLA extend                         mla_extend_attention.hip:224              :223, :227            mla_extend_attention.hip:250
  GQA decode   (4 / 8 waves)         decode_attention.hip:317                  :316, :320            decode_attention.hip:559 (the cross-wave
                                                                                                      merge :376-397 and the partials are f32)
  GQA extend   register-staged       extend_attention.hip:366                  :364, :369            extend_attention.hip:448
  GQA extend   LDS-DMA               extend_attention.hip:701                  (same order)          extend_attention.hip:764
  GQA extend   phased 32x32          extend_attention_phased.hip:330-331       :328-329, :418        extend_attention_phased.hip:437

Input conditions (asserted by the builders on the CPU before any launch): every row's visible logits lie within 8 nats (no P in the
f16 subnormals), every live reference mass exceeds 1e-5.  GQA queries are 0.5 * randn to stay inside the 8 nats at D = 128.

NEEDLE: q = 2 * k_needle (gap to every other logit >= 40 nats, asserted in float64): the needle's P is exactly 1 in every form that
takes its exponentials against the RUNNING maximum (all but the phased kernel), every other term is below e^-40, l = 1 +- 1e-5 and
the rounded output is the needle's value row bit for bit (no value element lies in (0, 2^-10)).  The phased 32x32 kernel
subtracts a deferred reference maximum inside the MFMA accumulation (extend_attention_phased.hip:203-206, :342, :372-387), so the
needle's P is 1 only up to f32 summation order: for it the relative bound of MASS is asserted against the needle's value row.
"""
import pytest
import torch

import _attn_positions as ap

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16"]
MAX_SPLITS = 8
MLA = (1, ap.MLA_D, ap.MLA_DV)
# a tile edge on both sides, empty splits, live splits of 64 keys, one key per value column at 512
MLA_DEC_SEQ = (1, 31, 32, 33, 97, 300, 512)
MLA_DEC_HQ = (1, 16, 20, 40, 80, 128)   # 20: WH = 2, second group partly dead; 40: WH = 4, one group partly and one wholly dead; 80: a second head block with one live group
MLA_WRAP_SEQ = (600, 40)                # past Dv = 512: a column sums two keys
# (prefix, extend): a tile edge on both sides of the seam, a tile that straddles it, a request with nothing to do, several row blocks
MLA_EXT_LENS = ((0, 1), (0, 33), (31, 5), (32, 32), (33, 70), (97, 3), (5, 0), (200, 130))
MLA_EXT_HQ = (1, 3, 8, 20, 128)         # 1 / 3 / 20: a 16-row group spans tokens in three different ways
GQA_DEC_SEQ = (1, 31, 32, 33, 97, 128)
GQA_DEC_HEADS = ((8, 2), (32, 8), (12, 12))
GQA_EXT_LENS = ((0, 1), (0, 33), (31, 5), (33, 70), (60, 64))
GQA_EXT_HEADS = ((8, 2), (3, 1), (14, 2))
DEC_MODES = {"auto": 0, "four_waves": 2, "eight_waves": 3}
EXT_MODES = {"register_staged": 0, "default": 1, "lds_dma": 3, "phased": 5}


def _mla(kind, lens, hq, dt):
    return (kind, lens, hq, *MLA, dt, ap.MLA_SCALE, 1.0)


def _gqa(kind, lens, hq, hkv, d, dt):
    return (kind, lens, hq, hkv, d, d, dt, d ** -0.5, 0.5)


def all_mass_problems():
    """Argument tuples of ap.mass_problem for every batch this module launches (the CPU suite checks each one's input conditions)."""
    out = []
    for dt in DTYPES:
        out += [_mla("decode", MLA_DEC_SEQ, hq, dt) for hq in MLA_DEC_HQ]
        out += [_mla("decode", MLA_WRAP_SEQ, 16, dt)]
        out += [_mla("extend", MLA_EXT_LENS, hq, dt) for hq in MLA_EXT_HQ]
        out += [_gqa("decode", GQA_DEC_SEQ, hq, hkv, 128, dt) for hq, hkv in GQA_DEC_HEADS] + [_gqa("decode", GQA_DEC_SEQ, 8, 2, 64, dt)]
        out += [_gqa("extend", GQA_EXT_LENS, hq, hkv, 128, dt) for hq, hkv in GQA_EXT_HEADS] + [_gqa("extend", GQA_EXT_LENS, 8, 2, 64, dt)]
    return out


def _needle_args(kind, lens, hq, hkv, d, dv, dt):
    # MLA: the model's scale; GQA D = 128: scale 1 (2 |k|^2 / sqrt(128) would leave a gap of only ~14 nats)
    return (kind, lens, hq, hkv, d, dv, dt, ap.MLA_SCALE if d == ap.MLA_D else 1.0)


def all_needle_problems():
    out = []
    for dt in DTYPES:
        out += [_needle_args("decode", MLA_DEC_SEQ, 128, *MLA, dt), _needle_args("extend", MLA_EXT_LENS, 128, *MLA, dt)]
        out += [_needle_args("decode", GQA_DEC_SEQ + (300,), 32, 8, 128, 128, dt), _needle_args("extend", GQA_EXT_LENS, 8, 2, 128, 128, dt)]
    return out


# ------------------------------------------------------------------------------------------------------------------ launching
WORST = {}   # (kernel form, dtype) -> worst |o - p| / p seen by this run


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst |o - p| / p per kernel form and dtype (bound: bf16 %.5f, f16 %.5f)" % (ap.tol_rel(torch.bfloat16), ap.tol_rel(torch.float16)))
    for (form, dt), w in sorted(WORST.items()):
        print(f"  {form:34s} {dt:5s} {w:.5f}")


def _assert_mass(form, dt, o, ref):
    tol = ap.tol_rel(ap._dt(dt), 2)
    ok, worst, bad = ap.check_mass(o.cpu(), ref, tol)
    WORST[(form, dt)] = max(WORST.get((form, dt), 0.0), worst)
    print(f"{form} {dt}: worst |o - p| / p = {worst:.5f} (bound {tol:.5f})")
    assert ok, f"{form} {dt}: {bad} elements outside tol_rel = {tol:.5f} (or non-zero where the mass is zero); worst relative error {worst:.5f}"


def _dev():
    return torch.device("cuda:0")


def _pools(P):
    k = P.kbuf.to(_dev())
    return k, (k[..., :P.dv] if P.mla else P.vbuf.to(_dev()))


def _splits(mode, bs):
    return {"one": [1] * bs, "ragged": [(i % 8) + 1 for i in range(bs)], "max": [MAX_SPLITS] * bs}[mode]


def _decode(P, q, splits, o=None):
    """decode_attention_fwd with NaN-prefilled output and split scratch; q / o may be strided device views."""
    from ltp_sglang_amd import sgl_kernel

    dev, bs = _dev(), len(P.lay)
    k, v = _pools(P)
    q = q.to(dev)
    if o is None:
        o = torch.full((bs, P.hq, P.dv), float("nan"), dtype=P.dtype, device=dev)
    logits = torch.full((bs, P.hq, MAX_SPLITS, P.dv), float("nan"), dtype=torch.float32, device=dev)
    lse = torch.full((bs, P.hq, MAX_SPLITS), float("nan"), dtype=torch.float32, device=dev)
    sgl_kernel.decode_attention_fwd(q, k, v, o, P.kv_indptr.to(dev), P.slots.to(dev), logits, lse,
                                    torch.tensor(splits, dtype=torch.int32, device=dev), MAX_SPLITS, P.scale)
    torch.cuda.synchronize()
    return o


def _extend(P, q, causal, o=None, ke=None):
    """extend_attention_fwd (qo_indptr mode) with a NaN-prefilled output; q / o / k_extend may be strided device views."""
    from ltp_sglang_amd import sgl_kernel

    dev = _dev()
    k, v = _pools(P)
    q = q.to(dev)
    ke = P.ke.to(dev) if ke is None else ke
    ve = ke[..., :P.dv] if P.mla else P.ve.to(dev)
    if o is None:
        o = torch.full((P.nq, P.hq, P.dv), float("nan"), dtype=P.dtype, device=dev)
    sgl_kernel.extend_attention_fwd(q, ke, ve, o, k, v, P.qo_indptr.to(dev), P.kv_indptr.to(dev), P.slots.to(dev), None, causal, None,
                                    max(e for _, e, _ in P.lay), P.scale)
    torch.cuda.synchronize()
    return o


def _decode_mode(mode):
    from ltp_sglang_amd import _cabi
    _cabi.check(_cabi.lib.sgl_mi355_decode_attention_set_mode(mode))


def _extend_mode(mode):
    from ltp_sglang_amd import _cabi
    _cabi.check(_cabi.lib.sgl_mi355_extend_attention_set_mode(mode))


def _padded(rows, width, pad, dtype, fill):
    """A [rows, width + pad] device buffer filled with `fill` and its [rows, width] view (row stride width + pad)."""
    buf = torch.full((rows, width + pad), fill, dtype=dtype, device=_dev())
    return buf, buf[:, :width]


# ------------------------------------------------------------------------------------------------------------------ 1. MASS
@pytest.mark.parametrize("split_mode", ["one", "ragged", "max"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hq", MLA_DEC_HQ)
def test_mla_decode_mass(hq, dt, split_mode, pkg):
    """Two roundings: P (mla_decode_attention.hip:211), the stage-2 store (decode_attention.hip:559)."""
    P = ap.mass_problem(*_mla("decode", MLA_DEC_SEQ, hq, dt))
    o = _decode(P, P.q, _splits(split_mode, len(P.lay)))
    _assert_mass("mla decode", dt, o, P.ref[False])


@pytest.mark.parametrize("dt", DTYPES)
def test_mla_decode_mass_wraps_past_dv(dt, pkg):
    """600 keys over 512 columns: 88 columns hold the summed mass of two keys (in different tiles and, split, different workgroups)."""
    P = ap.mass_problem(*_mla("decode", MLA_WRAP_SEQ, 16, dt))
    for split_mode in ("one", "max"):
        _assert_mass("mla decode", dt, _decode(P, P.q, _splits(split_mode, len(P.lay))), P.ref[False])


@pytest.mark.parametrize("table_dtype", [torch.int32, torch.int64], ids=["r2t32", "r2t64"])
@pytest.mark.parametrize("dt", DTYPES)
def test_mla_decode_mass_req_to_token_mode(dt, table_dtype, pkg):
    """sgl_kernel.decode_attention: the pool is addressed through req_to_token[req_pool_indices[b], :seq_lens[b]] (request_range's
    second mode) and the last key of every request is written by the call itself."""
    from ltp_sglang_amd import sgl_kernel

    hq, dev = 40, _dev()
    P = ap.mass_problem(*_mla("decode", MLA_DEC_SEQ, hq, dt))
    bs = len(P.lay)
    k, v = _pools(P)
    new = P.slots[(P.kv_indptr[1:] - 1).long()].long().to(dev)   # the slot of every request's last key
    rows = k[new].clone()
    k[new] = float("nan")
    perm = torch.tensor([5, 2, 9, 0, 7, 3, 8], dtype=torch.int64)   # request b's row of a larger table; the other rows point at slot 0
    table = torch.zeros((10, P.r2t.shape[1]), dtype=table_dtype)
    table[perm] = P.r2t.to(table_dtype)
    o = torch.full((bs, hq, P.dv), float("nan"), dtype=P.dtype, device=dev)
    scratch = torch.full((bs, hq, MAX_SPLITS, P.dv + 1), float("nan"), dtype=torch.float32, device=dev)
    seq = torch.tensor(MLA_DEC_SEQ, dtype=torch.int64, device=dev)
    sgl_kernel.decode_attention(P.q.to(dev), k, v, o, rows, rows[..., :P.dv], new, scratch, table.to(dev), perm.to(dev), seq, P.scale, 0.0)
    torch.cuda.synchronize()
    _assert_mass("mla decode (req_to_token)", dt, o, P.ref[False])


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hq", MLA_EXT_HQ)
def test_mla_extend_mass(hq, dt, causal, pkg):
    """Two roundings: P (mla_extend_attention.hip:224), the output store (:250)."""
    P = ap.mass_problem(*_mla("extend", MLA_EXT_LENS, hq, dt))
    _assert_mass("mla extend", dt, _extend(P, P.q, causal), P.ref[causal])


@pytest.mark.parametrize("dt", DTYPES)
def test_mla_extend_mass_req_to_token_mode(dt, pkg):
    """sgl_kernel.extend_attention: prefix through req_to_token, rows through extend_start_loc / extend_seq_lens; causal."""
    from ltp_sglang_amd import sgl_kernel

    hq, dev = 20, _dev()
    P = ap.mass_problem(*_mla("extend", MLA_EXT_LENS, hq, dt))
    k, v = _pools(P)
    ke = P.ke.to(dev)
    bs = len(P.lay)
    perm = torch.tensor([4, 0, 6, 1, 9, 3, 7, 2], dtype=torch.int64)
    table = torch.zeros((10, P.r2t.shape[1]), dtype=torch.int32)
    table[perm] = P.r2t
    seq = torch.tensor([a + e for a, e, _ in P.lay], dtype=torch.int64, device=dev)
    ext = torch.tensor([e for _, e, _ in P.lay], dtype=torch.int32, device=dev)
    o = torch.full((P.nq, hq, P.dv), float("nan"), dtype=P.dtype, device=dev)
    sgl_kernel.extend_attention(P.q.to(dev), ke, ke[..., :P.dv], o, k, v, table.to(dev), perm.to(dev), seq, ext,
                                P.qo_indptr[:bs].to(dev), int(ext.max()), P.scale, 0.0)
    torch.cuda.synchronize()
    _assert_mass("mla extend (req_to_token)", dt, o, P.ref[True])


@pytest.mark.parametrize("mode", list(DEC_MODES))
@pytest.mark.parametrize("split_mode", ["one", "ragged", "max"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hq,hkv,d", [(*h, 128) for h in GQA_DEC_HEADS] + [(8, 2, 64)])
def test_gqa_decode_mass(hq, hkv, d, dt, split_mode, mode, pkg):
    """Two roundings: P (decode_attention.hip:317), the stage-2 store (:559); the cross-wave merge (:376-397) is f32.  At D = 64
    the sequences of 97 and 128 keys wrap past Dv: those columns hold summed mass."""
    P = ap.mass_problem(*_gqa("decode", GQA_DEC_SEQ, hq, hkv, d, dt))
    try:
        _decode_mode(DEC_MODES[mode])
        o = _decode(P, P.q, _splits(split_mode, len(P.lay)))
    finally:
        _decode_mode(0)
    _assert_mass(f"gqa decode D={d} ({mode})", dt, o, P.ref[False])


@pytest.mark.parametrize("mode", list(EXT_MODES))
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hq,hkv,d", [(*h, 128) for h in GQA_EXT_HEADS] + [(8, 2, 64)])
def test_gqa_extend_mass(hq, hkv, d, dt, causal, mode, pkg):
    """Two roundings in each form: register-staged extend_attention.hip:366 / :448, LDS-DMA :701 / :764, phased
    extend_attention_phased.hip:330-331 / :437.  D = 64 is served by the register-staged kernel in every mode."""
    P = ap.mass_problem(*_gqa("extend", GQA_EXT_LENS, hq, hkv, d, dt))
    try:
        _extend_mode(EXT_MODES[mode])
        o = _extend(P, P.q, causal)
    finally:
        _extend_mode(1)
    _assert_mass(f"gqa extend D={d} ({mode})", dt, o, P.ref[causal])


# ---------------------------------------------------------------------------------------------------------------- 2. NEEDLE
def _bits(x):
    return x.contiguous().view(torch.int16)


@pytest.mark.parametrize("split_mode", ["one", "ragged", "max"])
@pytest.mark.parametrize("dt", DTYPES)
def test_mla_decode_needle(dt, split_mode, pkg):
    """Running maximum (mla_decode_attention.hip:201-209): P(needle) = 1, o = kv[slot, :512] bit for bit, through stage 2."""
    P = ap.needle_problem(*_needle_args("decode", MLA_DEC_SEQ, 128, *MLA, dt))
    for rnd in range(3):
        q, want = ap.needle_queries(P, rnd)
        o = _decode(P, q, _splits(split_mode, len(P.lay))).cpu()
        assert torch.equal(_bits(o), _bits(want)), f"round {rnd}: {int((_bits(o) != _bits(want)).any(-1).sum())} (request, head) rows differ"


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("dt", DTYPES)
def test_mla_extend_needle(dt, causal, pkg):
    """Running maximum (mla_extend_attention.hip:214-222): o = kv[slot, :512] or k_extend[row, :512] bit for bit; the needle of row t
    is one of the keys the row sees (<= pre + t when causal)."""
    P = ap.needle_problem(*_needle_args("extend", MLA_EXT_LENS, 128, *MLA, dt))
    for rnd in range(3):
        q, want = ap.needle_queries(P, rnd, causal)
        o = _extend(P, q, causal).cpu()
        assert torch.equal(_bits(o), _bits(want)), f"round {rnd}: {int((_bits(o) != _bits(want)).any(-1).sum())} (token, head) rows differ"


@pytest.mark.parametrize("mode", list(DEC_MODES))
@pytest.mark.parametrize("split_mode", ["one", "ragged", "max"])
@pytest.mark.parametrize("dt", DTYPES)
def test_gqa_decode_needle(dt, split_mode, mode, pkg):
    """Running maximum (decode_attention.hip:307-315), f32 cross-wave merge and stage 2: the needle's value row bit for bit.
    Hq = 32 over sequences up to 300: rounds 0..9 make every position a needle."""
    P = ap.needle_problem(*_needle_args("decode", GQA_DEC_SEQ + (300,), 32, 8, 128, 128, dt))
    try:
        _decode_mode(DEC_MODES[mode])
        for rnd in range(10):
            q, want = ap.needle_queries(P, rnd)
            o = _decode(P, q, _splits(split_mode, len(P.lay))).cpu()
            assert torch.equal(_bits(o), _bits(want)), f"round {rnd}: {int((_bits(o) != _bits(want)).any(-1).sum())} rows differ"
    finally:
        _decode_mode(0)


@pytest.mark.parametrize("mode", list(EXT_MODES))
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("dt", DTYPES)
def test_gqa_extend_needle(dt, causal, mode, pkg):
    """Register-staged and LDS-DMA kernels take exponentials against the running maximum (extend_attention.hip:355-363, :693-699):
    bit equality.  The phased kernel's deferred reference maximum enters the MFMA accumulation (extend_attention_phased.hip:342),
    so its needle P is 1 only up to f32 summation order: the relative bound of MASS (two roundings) against the needle's row."""
    P = ap.needle_problem(*_needle_args("extend", GQA_EXT_LENS, 8, 2, 128, 128, dt))
    try:
        _extend_mode(EXT_MODES[mode])
        for rnd in range(17):   # Hq = 8, up to 124 visible keys
            q, want = ap.needle_queries(P, rnd, causal)
            o = _extend(P, q, causal).cpu()
            if mode == "phased":
                err = (o.double() - want.double()).abs()
                assert bool((err <= ap.tol_rel(P.dtype) * want.double().abs() + ap.TINY).all()), f"round {rnd}: worst {err.max().item():.3e}"
            else:
                assert torch.equal(_bits(o), _bits(want)), f"round {rnd}: {int((_bits(o) != _bits(want)).any(-1).sum())} rows differ"
    finally:
        _extend_mode(1)


# --------------------------------------------------------------------------------------------------------------- 3. STRIDES
SENTINEL = 7.0


@pytest.mark.parametrize("dt", DTYPES)
def test_mla_decode_mass_strided_q_and_o(dt, pkg):
    """q: token stride Hq * 576 + 64 (NaN padding); o: token stride Hq * 512 + 32, whose padding must come back untouched."""
    hq = 20
    P = ap.mass_problem(*_mla("decode", MLA_DEC_SEQ, hq, dt))
    bs = len(P.lay)
    _, qv = _padded(bs, hq * P.d, 64, P.dtype, float("nan"))
    qv.copy_(P.q.reshape(bs, -1))
    obuf, ov = _padded(bs, hq * P.dv, 32, P.dtype, SENTINEL)
    _decode(P, qv.view(bs, hq, P.d), _splits("ragged", bs), o=ov.view(bs, hq, P.dv))
    assert bool((obuf[:, hq * P.dv:] == SENTINEL).all())
    _assert_mass("mla decode (strided)", dt, ov.reshape(bs, hq, P.dv), P.ref[False])


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("dt", DTYPES)
def test_mla_extend_mass_strided_q_k_and_o(dt, causal, pkg):
    """q: token stride Hq * 576 + 64; k_extend: token stride 576 + 64 (both NaN-padded); o: token stride Hq * 512 + 32 (sentinel)."""
    hq = 20
    P = ap.mass_problem(*_mla("extend", MLA_EXT_LENS, hq, dt))
    t = P.nq
    _, qv = _padded(t, hq * P.d, 64, P.dtype, float("nan"))
    qv.copy_(P.q.reshape(t, -1))
    _, kv = _padded(t, P.d, 64, P.dtype, float("nan"))
    kv.copy_(P.ke.reshape(t, -1))
    obuf, ov = _padded(t, hq * P.dv, 32, P.dtype, SENTINEL)
    _extend(P, qv.view(t, hq, P.d), causal, o=ov.view(t, hq, P.dv), ke=kv.unsqueeze(1))
    assert bool((obuf[:, hq * P.dv:] == SENTINEL).all())
    _assert_mass("mla extend (strided)", dt, ov.reshape(t, hq, P.dv), P.ref[causal])
