"""CPU checks of the position-resolved attention tests themselves (no GPU): the comparator accepts an emulation of the kernels'
arithmetic inside the derived bound, rejects every emulated indexing mistake, and the input builders meet the conditions the
bound rests on for every shape test_attention_positions_gpu.py launches."""
import pytest
import torch

import _attn_positions as ap
import test_attention_positions_gpu as gpu_cases

DTYPES = ["bf16", "f16"]
# decode lengths: the four the emulation is checked at, and one key more than 300 / 512 for the causal-limit mutations
EMU_LENS = (1, 33, 300, 512, 301, 513)


def _emu_problem(dtype_name):
    return ap.mass_problem("decode", EMU_LENS, 16, 1, ap.MLA_D, ap.MLA_DV, dtype_name, ap.MLA_SCALE, pool=2048, keep_logits=True)


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("req", [0, 1, 2, 3], ids=["len1", "len33", "len300", "len512"])
def test_emulated_arithmetic_passes_the_comparator(req, dtype_name):
    """The reference stays inside the derived bound: f32 scores, P to dtype, f32 accumulate, one rounded output -- two roundings."""
    P = _emu_problem(dtype_name)
    s = P.logits[(req, False)][0]                       # [hq, n]
    o = ap.emulate_mass(s, ap.MLA_DV, P.dtype)
    ok, worst, bad = ap.check_mass(o, P.ref[False][req], ap.tol_rel(P.dtype))
    print(f"emulation len={EMU_LENS[req]} {dtype_name}: worst |o - p| / p = {worst:.5f}, bound {ap.tol_rel(P.dtype):.5f}")
    assert ok, f"{bad} elements outside the bound, worst {worst}"


def _mutations(n):
    """name -> (weight, cols) of an emulated kernel that mishandles one key of an n-key row."""
    out = {}
    for name, key, w in (("drop_middle", n // 2, 0.0), ("drop_last", n - 1, 0.0), ("twice", n // 2 + 1, 2.0)):
        weight = torch.ones(n)
        weight[key] = w
        out[name] = (weight, None)
    return out


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("req", [2, 3], ids=["len300", "len512"])
@pytest.mark.parametrize("mutation", ["drop_middle", "drop_last", "twice", "swap_rows"])
def test_comparator_rejects_a_mishandled_key(mutation, req, dtype_name):
    P = _emu_problem(dtype_name)
    s = P.logits[(req, False)][0]
    n = s.shape[-1]
    if mutation == "swap_rows":   # two rows of one 32-key tile change places in the value image: in every head, P of one lands in the other's column
        tile = s[0, 64:96]
        i, j = 64 + int(tile.argmax()), 64 + int(tile.argmin())
        cols = torch.arange(n) % ap.MLA_DV
        cols[i], cols[j] = cols[j].clone(), cols[i].clone()
        o = ap.emulate_mass(s, ap.MLA_DV, P.dtype, cols=cols)
    else:
        weight, cols = _mutations(n)[mutation]
        o = ap.emulate_mass(s, ap.MLA_DV, P.dtype, weight=weight, cols=cols)
    ok, worst, bad = ap.check_mass(o, P.ref[False][req], ap.tol_rel(P.dtype))
    print(f"{mutation} len={n} {dtype_name}: worst |o - p| / p = {worst:.4f}, {bad} elements flagged")
    assert not ok and bad >= 1


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("req", [4, 5], ids=["limit300", "limit512"])
@pytest.mark.parametrize("delta", [-1, 1], ids=["one_short", "one_over"])
def test_comparator_rejects_a_causal_limit_off_by_one(delta, req, dtype_name):
    """The last row sees keys [0, lim) of a stream one key longer; the emulated kernel masks at lim + delta."""
    P = _emu_problem(dtype_name)
    raw = P.logits[(req, False)][0]
    lim = raw.shape[-1] - 1
    keys = torch.arange(lim + 1)
    ref = ap.mass_of(raw.masked_fill(keys >= lim, float("-inf")), ap.MLA_DV)
    good = ap.emulate_mass(raw.masked_fill(keys >= lim, float("-inf")), ap.MLA_DV, P.dtype)
    assert ap.check_mass(good, ref, ap.tol_rel(P.dtype))[0]
    o = ap.emulate_mass(raw.masked_fill(keys >= lim + delta, float("-inf")), ap.MLA_DV, P.dtype)
    ok, worst, bad = ap.check_mass(o, ref, ap.tol_rel(P.dtype))
    assert not ok and bad >= 1


def test_comparator_wants_exact_zeros_and_rejects_nan():
    p = torch.tensor([[0.75, 0.25, 0.0]], dtype=torch.float64)
    assert ap.check_mass(torch.tensor([[0.75, 0.25, 0.0]]), p, 2.0 ** -7)[0]
    assert not ap.check_mass(torch.tensor([[0.75, 0.25, 1e-30]]), p, 2.0 ** -7)[0]
    assert not ap.check_mass(torch.tensor([[0.75, float("nan"), 0.0]]), p, 2.0 ** -7)[0]
    assert not ap.check_mass(torch.tensor([[0.75, 0.25, float("nan")]]), p, 2.0 ** -7)[0]
    assert not ap.check_mass(torch.tensor([[0.75, 0.25 * (1 + 2.0 ** -6), 0.0]]), p, 2.0 ** -7)[0]


@pytest.mark.parametrize("args", gpu_cases.all_mass_problems(), ids=lambda a: "-".join(str(x) for x in (a[0], a[2], a[3], a[4], a[6])))
def test_mass_builders_meet_the_input_conditions(args):
    P = ap.mass_problem(*args)          # asserts spread and minimum mass
    print(f"{args[0]} hq={args[2]} hkv={args[3]} d={args[4]} {args[6]}: spread {P.spread:.2f} nats, smallest live mass {P.min_mass:.2e}")
    assert P.spread <= ap.MAX_SPREAD and P.min_mass > ap.MIN_MASS
    for causal, ref in P.ref.items():   # a row's masses sum to one; a causal row leaves the columns of unseen keys exactly zero
        live = ref.sum(-1) > 0
        assert torch.allclose(ref.sum(-1)[live], torch.ones(int(live.sum()), dtype=torch.float64), atol=1e-12)


@pytest.mark.parametrize("args", gpu_cases.all_needle_problems(), ids=lambda a: "-".join(str(x) for x in (a[0], a[2], a[3], a[4], a[6])))
def test_needle_builders_meet_the_input_conditions(args):
    P = ap.needle_problem(*args)        # asserts the gap
    print(f"{args[0]} hq={args[2]} hkv={args[3]} d={args[4]} {args[6]}: needle gap {P.gap:.1f} nats")
    assert P.gap >= ap.MIN_GAP
    v = torch.cat([P.vbuf[P.slots.long()].float().flatten()] + ([P.ve.float().flatten()] if P.ve is not None else []))
    assert not ((v != 0) & (v.abs() < ap.V_FLOOR)).any()
    q, want = ap.needle_queries(P, 1, causal=P.kind == "extend")
    assert torch.isfinite(q.float()).all() and torch.isfinite(want.float()).all()


def test_needle_rounds_cover_every_position():
    """Hq = 128, rounds 0..2: every position of every sequence up to 300 keys is the needle of some head."""
    for n in (1, 31, 32, 33, 97, 300):
        hit = {(h + 128 * r) % n for r in range(3) for h in range(128)}
        assert hit == set(range(n))
