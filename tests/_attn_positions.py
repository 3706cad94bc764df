"""CPU side of the position-resolved attention tests (test_attention_positions_gpu.py, test_attention_positions.py).

Two input constructions make every single key visible in the output of an attention kernel:

* MASS.  The value row of the key at sequence position j is the one-hot of column j mod Dv, so o[.., c] IS the softmax mass of the
  keys with j mod Dv == c and the float64 softmax is the reference.  For the 576 / 512 latent (MLA) rows the value is the first
  512 columns of the key row itself: columns 0..511 are the one-hot, columns 512..575 are randn, so the logit of key j is
  scale * (q[j mod 512] + q_rope . k_rope_j) -- a K fragment read from the wrong chunk picks another q element.
* NEEDLE.  q = 2 * k_needle makes one key's probability exactly 1 and every other one vanish, so the output row is the needle's
  value row bit for bit.

Everything here is plain torch on the CPU: builders (which assert the input conditions the derived tolerances rest on), the
float64 references, the comparator, and a small emulation of the kernels' arithmetic with which the comparator is tested.
"""
import functools
from types import SimpleNamespace

import torch

HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # relative cost of one rounding to the 16-bit type
F32_TERM = 2.0 ** -12    # exp2 approximation + the rounded scale * log2 e product (about 1e-6 at these logits): a wide margin
TINY = 1e-9              # absolute slack of the comparator, four decades under the smallest live mass it ever scales
MAX_SPREAD = 8.0         # nats between a row's largest and smallest visible logit: no P falls into the f16 subnormals
MIN_MASS = 1e-5          # every live reference mass is above this
MIN_GAP = 40.0           # nats between the needle's logit and the next one
V_FLOOR = 2.0 ** -10     # no needle value element sits in (0, V_FLOOR): a 1e-5 relative wobble cannot cross a rounding boundary

MLA_D, MLA_DV = 576, 512
MLA_SCALE = 192 ** -0.5


def tol_rel(dtype, roundings=2):
    """(roundings to the 16-bit type between score and output) x half an ulp + the f32 term.  Derived, not fitted."""
    return roundings * HALF_ULP[dtype] + F32_TERM


# ---------------------------------------------------------------------------------------------------------------- comparator
def mass_of(logits, dv, cols=None):
    """float64 softmax over the last axis (masked keys are -inf), summed into column j mod dv: [..., n] -> [..., dv]."""
    n = logits.shape[-1]
    p = torch.softmax(logits.double(), dim=-1)
    cols = torch.arange(n) % dv if cols is None else cols
    flat = p.reshape(-1, n)
    return torch.zeros(flat.shape[0], dv, dtype=torch.float64).index_add_(1, cols, flat).reshape(*logits.shape[:-1], dv)


def check_mass(o, p, tol):
    """|o - p| <= tol * p + TINY where the reference mass p is positive; exactly 0.0 where it is exactly zero (masked causal
    keys, columns without a key).  NaN fails both.  -> (ok, worst |o - p| / p over the live elements, number of bad elements)."""
    o = o.double()
    assert o.shape == p.shape, (o.shape, p.shape)
    zero = p == 0
    err = (o - p).abs()
    bad = torch.where(zero, o != 0, ~(err <= tol * p + TINY))
    live = ~zero
    rel = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err) / torch.where(live, p, torch.ones_like(p))
    worst = rel[live].max().item() if live.any() else 0.0
    return not bool(bad.any()), worst, int(bad.sum())


def emulate_mass(logits, dv, dtype, weight=None, cols=None):
    """The kernels' arithmetic on one-hot values: f32 scores, P = exp(s - max) in f32, the row sum of the UNROUNDED P, P rounded
    to the value dtype, f32 accumulation, one rounding of acc / l.  weight: how often each key is counted (0 = dropped,
    2 = counted twice); cols: the value column each key's P lands in (a swapped tile row)."""
    s = logits.float()
    n = s.shape[-1]
    w = torch.ones(n) if weight is None else weight.float()
    cols = torch.arange(n) % dv if cols is None else cols
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    l = (p * w).sum(-1, keepdim=True)
    pr = (p.to(dtype).float() * w).reshape(-1, n)
    acc = torch.zeros(pr.shape[0], dv).index_add_(1, cols, pr).reshape(*s.shape[:-1], dv)
    return (acc / l).to(dtype)


# ------------------------------------------------------------------------------------------------------------------ builders
def _dt(name):
    return {"bf16": torch.bfloat16, "f16": torch.float16}[name]


def _layout(kind, lens):
    """-> per request (keys in the pool, keys in k_extend, query rows).  decode: lens = seq lens; extend: lens = (prefix, extend)."""
    if kind == "decode":
        return [(n, 0, 1) for n in lens]
    return [(p, e, e) for p, e in lens]


def _indptr(counts):
    out = torch.zeros(len(counts) + 1, dtype=torch.int32)
    out[1:] = torch.cumsum(torch.tensor(counts), 0)
    return out


def _floor_small(x):
    f = x.float()
    small = (f != 0) & (f.abs() < V_FLOOR)
    return torch.where(small, torch.sign(f) * V_FLOOR, f).to(x.dtype)


def _base(kind, lens, hq, hkv, d, dv, dtype, pool, seed, one_hot):
    """Pool, k_extend and index tensors of one batch.  The pool is permuted, row 0 is finite and never referenced (the kernels
    read it for dead tile rows), every other unreferenced row is NaN.  one_hot: value rows are the one-hot of their position
    (MASS), else randn with the small elements floored (NEEDLE).  MLA (d, dv) = (576, 512): the value IS k[..., :512]."""
    mla = (d, dv) == (MLA_D, MLA_DV)
    assert not mla or hkv == 1
    g = torch.Generator().manual_seed(seed)
    lay = _layout(kind, lens)
    npre, t = sum(a for a, _, _ in lay), sum(e for _, e, _ in lay)
    assert npre <= pool - 1
    slots = torch.randperm(pool - 1, generator=g)[:npre] + 1
    kv_indptr, qo_indptr = _indptr([a for a, _, _ in lay]), _indptr([e for _, e, _ in lay])
    pos_pool = torch.cat([torch.arange(a) for a, _, _ in lay]) if npre else torch.zeros(0, dtype=torch.int64)
    pos_ext = torch.cat([a + torch.arange(e) for a, e, _ in lay]) if t else torch.zeros(0, dtype=torch.int64)

    def rows(n, positions):
        k = torch.randn(n, hkv, d, generator=g).to(dtype)
        v = None if mla else torch.randn(n, hkv, dv, generator=g).to(dtype)
        tgt = k[..., :dv] if mla else v
        if positions is None:            # the pool before its referenced rows are placed: finite garbage, floored like the rest
            if not one_hot:
                tgt.copy_(_floor_small(tgt))
        elif one_hot:
            tgt.copy_(torch.nn.functional.one_hot(positions % dv, dv).to(dtype).unsqueeze(1).expand(n, hkv, dv))
        else:
            tgt.copy_(_floor_small(tgt))
        return k, (k[..., :dv] if mla else v)

    kbuf, vbuf = rows(pool, None)
    kp, vp = rows(npre, pos_pool)
    kbuf[slots] = kp
    if not mla:
        vbuf[slots] = vp
    dead = torch.ones(pool, dtype=torch.bool)
    dead[slots] = False
    dead[0] = False
    kbuf[dead] = float("nan")
    if not mla:
        vbuf[dead] = float("nan")
    ke, ve = rows(t, pos_ext) if kind == "extend" else (None, None)
    r2t = torch.zeros(len(lay), max(1, max(a + e for a, e, _ in lay)), dtype=torch.int32)
    for b, (a, _, _) in enumerate(lay):
        r2t[b, :a] = slots[kv_indptr[b]: kv_indptr[b + 1]]
    P = SimpleNamespace(kind=kind, lens=list(lens), lay=lay, hq=hq, hkv=hkv, d=d, dv=dv, dtype=dtype, mla=mla, gen=g,
                        kbuf=kbuf, vbuf=vbuf, ke=ke, ve=ve, slots=slots.int(), kv_indptr=kv_indptr, qo_indptr=qo_indptr, r2t=r2t,
                        nq=sum(q for _, _, q in lay), q_indptr=_indptr([q for _, _, q in lay]))
    return P


def _stream(P, b):
    """The key / value rows request b attends over, in sequence order: pool rows, then its k_extend rows."""
    s = P.slots[P.kv_indptr[b]: P.kv_indptr[b + 1]].long()
    k, v = P.kbuf[s], P.vbuf[s]
    if P.ke is not None:
        e = slice(int(P.qo_indptr[b]), int(P.qo_indptr[b + 1]))
        k, v = torch.cat([k, P.ke[e]]), torch.cat([v, P.ve[e]])
    return k, v


def _limits(P, b, causal):
    """Keys [0, lim) each query row of request b sees."""
    a, e, nq = P.lay[b]
    if P.kind == "extend" and causal:
        return a + 1 + torch.arange(nq)
    return torch.full((nq,), a + e)


def _logits(P, b, q, scale):
    """float64 logits [nq, hq, n] of request b's query rows q [nq, hq, d] against its whole key stream (one gemm per kv head)."""
    k = _stream(P, b)[0].double()
    grp = P.hq // P.hkv
    nq = q.shape[0]
    out = [(q[:, h * grp:(h + 1) * grp].double().reshape(nq * grp, P.d) @ k[:, h].T).view(nq, grp, -1) for h in range(P.hkv)]
    return torch.cat(out, 1) * scale


@functools.lru_cache(maxsize=None)
def mass_problem(kind, lens, hq, hkv, d, dv, dtype_name, scale, q_std=1.0, pool=1024, seed=0, keep_logits=False):
    """One MASS batch and its float64 references (P.ref[causal]: [rows, hq, dv]).  Asserts the input conditions:
    every row's visible logits lie within MAX_SPREAD nats, every live reference mass exceeds MIN_MASS."""
    dtype = _dt(dtype_name)
    P = _base(kind, lens, hq, hkv, d, dv, dtype, pool, seed + 1000 * hq, True)
    P.scale = scale
    P.q = (q_std * torch.randn(P.nq, hq, d, generator=P.gen)).to(dtype)
    P.ref, P.spread, P.min_mass, P.logits = {}, 0.0, 1.0, {}
    for causal in ((False, True) if kind == "extend" else (False,)):
        ref = torch.zeros(P.nq, hq, dv, dtype=torch.float64)
        for b, (_, _, nq) in enumerate(P.lay):
            if nq == 0:
                continue
            r = slice(int(P.q_indptr[b]), int(P.q_indptr[b + 1]))
            s = _logits(P, b, P.q[r], scale)
            vis = torch.arange(s.shape[-1]).view(1, 1, -1) < _limits(P, b, causal).view(-1, 1, 1)
            P.spread = max(P.spread, (s.masked_fill(~vis, -1e300).amax(-1) - s.masked_fill(~vis, 1e300).amin(-1)).max().item())
            s = s.masked_fill(~vis, float("-inf"))
            ref[r] = mass_of(s, dv)
            if keep_logits:
                P.logits[(b, causal)] = s
        P.ref[causal] = ref
        P.min_mass = min(P.min_mass, ref[ref > 0].min().item())
    assert P.spread <= MAX_SPREAD, f"logit spread {P.spread:.2f} nats"
    assert P.min_mass > MIN_MASS, f"smallest live mass {P.min_mass:.2e}"
    return P


@functools.lru_cache(maxsize=None)
def needle_problem(kind, lens, hq, hkv, d, dv, dtype_name, scale, pool=1024, seed=0):
    """One NEEDLE batch: randn keys, value elements floored at V_FLOOR.  Asserts that for EVERY key of every request taken as the
    needle (q = 2 k) its logit exceeds every other key's by MIN_GAP nats -- over the whole stream, so also over any causal part."""
    dtype = _dt(dtype_name)
    P = _base(kind, lens, hq, hkv, d, dv, dtype, pool, seed + 7, False)
    P.scale, P.gap = scale, float("inf")
    for b in range(len(P.lay)):
        k = _stream(P, b)[0].double()
        for h in range(hkv):
            gram = 2.0 * scale * (k[:, h] @ k[:, h].T)
            diag = gram.diagonal().clone()
            gram.fill_diagonal_(float("-inf"))
            if gram.shape[0] > 1:
                P.gap = min(P.gap, (diag - gram.amax(-1)).min().item())
    assert P.gap >= MIN_GAP, f"needle gap {P.gap:.1f} nats"
    return P


def needle_queries(P, rnd, causal=False):
    """Round rnd: row (b, t), head h looks for the key at position (h + Hq * rnd) mod (keys the row sees).
    -> (q [rows, hq, d] = 2 * k_needle rounded to dtype, the expected output rows [rows, hq, dv] = the needle's value row)."""
    q = torch.zeros(P.nq, P.hq, P.d, dtype=P.dtype)
    want = torch.zeros(P.nq, P.hq, P.dv, dtype=P.dtype)
    kh = torch.arange(P.hq) // (P.hq // P.hkv)
    for b, (_, _, nq) in enumerate(P.lay):
        if nq == 0:
            continue
        k, v = _stream(P, b)
        pos = (torch.arange(P.hq).view(1, -1) + P.hq * rnd) % _limits(P, b, causal).view(-1, 1)   # [nq, hq]
        r = slice(int(P.q_indptr[b]), int(P.q_indptr[b + 1]))
        q[r] = (2.0 * k[pos, kh.view(1, -1)].float()).to(P.dtype)
        want[r] = v[pos, kh.view(1, -1)]
    return q, want
