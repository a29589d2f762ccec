"""-m gpu: the DPM++ SDE stage kernel (include/cfgpp_dpmpp_sde.h; csrc/dpmpp_sde_kernels.hip) - cfgpp_step_sde_stage bit for bit
against torch evaluating the header's expression sequence (tests/dpmpp_sde_ref.py: stage) on torch-CPU and on torch-ROCm, the
in-register noise against cfgpp_philox_normal's fill (stream 3), stage B's n1 against stage A's, the correlation of the two stages'
noise, chain independence past the 32 keys of one launch, and the library's refusals.

Like tests/test_gpu_sde_step.py every output carries guard elements that must stay untouched, outputs are NaN-filled before the call,
every tensor the stage must NOT read (the noise of a term that is off, x of a last stage whose base is another tensor, outputs)
holds NaN and every coefficient of a term that is off is finite and wrong, so a term that is evaluated although it is skipped shows;
torch-ROCm is asked on tensors padded to whole 4096-element blocks (see tests/test_gpu_vpred.py's docstring).  Coefficients are those
of real steps - the first, a middle and the next-to-last step of a 6-step Karras schedule at eta = 1 - so the magnitudes are the
product's.  Shapes: one group, a ragged last block (4 * 257), the grid-stride loop's second pass (4 * (262144 + 3): one launch
carries 1024 blocks of 256 threads), B = 33."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dpmpp_sde_ref as S

pytestmark = pytest.mark.gpu

H, F = torch.float16, torch.float32
GUARD = 64
SENTINEL = 1234.0
NAN = float("nan")
SEEDS = [0x0123456789ABCDEF, 7, (1 << 63) + 12345]
BIG = 4 * (262144 + 3)


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from cfgpp_amd import engine
    return engine


def _rand(shape, seed, scale=1.0, dtype=F):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _guarded(x, fill=SENTINEL):
    """a device copy of x followed by GUARD elements of ``fill`` -> (whole buffer, the view of x)"""
    n = x.numel()
    buf = torch.full((n + GUARD,), fill, dtype=x.dtype)
    buf[:n] = x.flatten()
    buf = buf.cuda()
    return buf, buf[:n].view(x.shape)


def _tail_ok(buf, n, fill=SENTINEL):
    t = buf[n:].float().cpu()
    return bool(torch.isnan(t).all()) if math.isnan(fill) else bool((t == fill).all())


def _on_rocm(fn, *tensors):
    n = tensors[0].numel()
    L = (n // 4096 + 2) * 4096
    dev = [None if t is None else torch.cat([t.flatten(), torch.zeros(L - n, dtype=t.dtype)]).cuda() for t in tensors]
    return tuple(o[:n].cpu() for o in fn(*dev))


def _sigmas():
    from cfgpp_amd.schedule import SchedulerTables
    return SchedulerTables(6).karras_sigmas()


def _row(i, stage, cfgpp, eta=1.0):
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_coeffs
    return dpmpp_sde_coeffs(_sigmas(), i, stage, eta, 1.0, cfgpp)


# how the buffers of a launch relate: base is x or its own tensor, out is x or its own tensor, den_out its own tensor or base
ALIASES = [dict(base_is_x=True, inplace=False), dict(base_is_x=True, inplace=True), dict(base_is_x=False, inplace=False),
           dict(base_is_x=False, inplace=True), dict(base_is_x=False, inplace=True, den_is_base=True)]


def _options(full=True):
    out = []
    for i in (0, 2, 4):                       # first / middle / next to last step of the 6-step schedule
        for stage in "AB":
            for cfgpp in (False, True):
                for al in (ALIASES if full else ALIASES[1:2] if stage == "A" else ALIASES[4:]):
                    out.append(dict(i=i, stage=stage, cfgpp=cfgpp, **al))
    for cfgpp in (False, True):
        for al in ALIASES[:3]:
            out.append(dict(i=4, stage="A", cfgpp=cfgpp, last=True, **al))
        out.append(dict(i=5, stage="A", cfgpp=cfgpp, **ALIASES[1]))                                # the schedule's own last row: zeros
        out.append(dict(i=5, stage="A", cfgpp=cfgpp, no_xc=True, **ALIASES[1]))                    # ... as the solver launches it
        for stage in "AB":
            out.append(dict(i=2, stage=stage, cfgpp=cfgpp, eta=0.0, **ALIASES[4 if stage == "B" else 0]))   # no noise term
            out.append(dict(i=2, stage=stage, cfgpp=cfgpp, single=True, **ALIASES[2]))
            out.append(dict(i=2, stage=stage, cfgpp=cfgpp, no_xc=True, **ALIASES[3]))
    return out


def _run_case(E, B, row, o, k):
    r = _row(o["i"], o["stage"], o["cfgpp"], o.get("eta", 1.0))
    coef, terms, last = list(r.coef), r.terms, bool(r.last or o.get("last"))
    # what a skipped term leaves unused is finite and wrong on purpose: it must play no part
    for bit, j, wrong in ((S.TERM_D, 2, 3.0), (S.TERM_U, 3, -2.0), (S.TERM_N1, 4, 5.0), (S.TERM_N2, 5, 7.0)):
        if last or not terms & bit:
            coef[j] = wrong
    n1_on, n2_on = (not last and bool(terms & S.TERM_N1)), (not last and bool(terms & S.TERM_N2))
    lam = 0.6 if o["cfgpp"] else 7.5
    single, base_is_x, inplace = bool(o.get("single")), o["base_is_x"], o["inplace"]
    seed = 1000 * k + row % 97 + B
    scale = float(coef[0]) if coef[0] > 1 else 1.3
    base = _rand((B, row), seed, scale)
    x = base if base_is_x else (torch.full((B, row), NAN) if last else _rand((B, row), seed + 6, scale))
    m_uc = _rand((B, row), seed + 1, dtype=H)
    m_c = m_uc if single else _rand((B, row), seed + 2, dtype=H)
    n1 = _rand((B, row), seed + 3) if n1_on else torch.full((B, row), NAN)
    n2 = _rand((B, row), seed + 4) if n2_on else torch.full((B, row), NAN)
    ref = lambda a, b, c, d, e, f_: S.stage(a, b, c, c if single else d, lam, coef, terms, last, e, f_, single=single)  # noqa: E731
    w = ref(x, base, m_uc, m_c, n1, n2)                                                      # torch-CPU
    g = _on_rocm(ref, x, base, m_uc, m_c, n1, n2)                                            # torch-ROCm
    n = B * row
    xb, xv = _guarded(x)
    bb, bv = (xb, xv) if base_is_x else _guarded(base)
    ob, ov = _guarded(torch.full((B, row), NAN))
    db, dv = _guarded(torch.full((B, row), NAN))
    cb, cv = _guarded(torch.full((B, row), NAN, dtype=H))
    ub, uv = _guarded(m_uc, NAN)
    mb, mv = (ub, uv) if single else _guarded(m_c, NAN)
    n1b, n1v = _guarded(n1, NAN)
    n2b, n2v = _guarded(n2, NAN)
    out = xv if inplace else ov
    den_out = bv if o.get("den_is_base") else dv
    xc_out = None if o.get("no_xc") else cv
    E.step_sde_stage(xv, bv, out, den_out, xc_out, uv, mv, lam, coef, terms, last, noise1=n1v if n1_on else None,
                     noise2=n2v if n2_on else None)
    torch.cuda.synchronize()
    got = [den_out.cpu(), out.cpu(), None if xc_out is None else cv.cpu()]
    bad = []
    for name, r_ in (("cpu", w), ("rocm", g)):
        for what, a, b in zip(("den", "out", "xc"), got, r_):
            if a is None:
                continue
            assert bool(torch.isfinite(a.float()).all()), (what, o)
            d = int((a.flatten() != b.flatten().to(a.dtype)).sum()) if a.dtype == b.dtype else -1
            if d:
                bad.append((name, what, d))
    if last:
        assert torch.equal(got[0], got[1])                              # out = den
    # guards: nothing is written past the end of any buffer, inputs are left alone, unused outputs stay NaN
    for buf, fill in ((xb, SENTINEL), (bb, SENTINEL), (ob, SENTINEL), (db, SENTINEL), (cb, SENTINEL), (ub, NAN), (mb, NAN), (n1b, NAN),
                      (n2b, NAN)):
        assert _tail_ok(buf, n, fill), o
    assert torch.equal(uv.cpu(), m_uc) and torch.equal(mv.cpu(), m_c)
    assert torch.equal(n1v.cpu(), n1) or not n1_on
    assert torch.equal(n2v.cpu(), n2) or not n2_on
    if not inplace and not (last and not base_is_x):
        assert torch.equal(xv.cpu(), x)
    if not base_is_x and not o.get("den_is_base"):
        assert torch.equal(bv.cpu(), base)
    if inplace:
        assert bool(torch.isnan(ov.cpu()).all())
    if o.get("den_is_base"):
        assert bool(torch.isnan(dv.cpu()).all())
    if o.get("no_xc"):
        assert bool(torch.isnan(cv.float().cpu()).all())
    return bad


@pytest.mark.parametrize("B,row", [(1, 4), (3, 4), (1, 4 * 257), (3, 4 * 257)])
def test_stage_equals_torch_bit_for_bit(E, B, row):
    bad = []
    for k, o in enumerate(_options()):
        for item in _run_case(E, B, row, o, k):
            bad.append((o, item))
    assert not bad, bad[:6]


def test_stage_equals_torch_bit_for_bit_on_the_second_grid_pass(E):
    """row_elems = 4 * (262144 + 3): three groups past what one pass of the 1024 x 256 threads covers; the solver's launches only"""
    opts = [dict(i=2, stage="A", cfgpp=False, **ALIASES[0]), dict(i=2, stage="B", cfgpp=True, **ALIASES[4]),
            dict(i=5, stage="A", cfgpp=True, no_xc=True, **ALIASES[1])]
    bad = []
    for k, o in enumerate(opts):
        for item in _run_case(E, 1, BIG, o, k):
            bad.append((o, item))
    assert not bad, bad


def _noise_only(E, B, row, seeds, draw1, draw2, terms, c1=1.0, c2=1.0, noise1=None, noise2=None, stage_b=False):
    """a launch on x = 0, m = 0: den = 0 and out = c_1 n1 + c_2 n2 of the terms that are on, nothing else (0 + v = v exactly).
    ``stage_b``: base is another (zero) tensor and the launch is in place, as the solver's stage B"""
    xb, xv = _guarded(torch.zeros(B, row))
    bb, bv = _guarded(torch.zeros(B, row)) if stage_b else (xb, xv)
    ob, ov = _guarded(torch.full((B, row), NAN))
    db, dv = _guarded(torch.full((B, row), NAN))
    m = torch.zeros(B, row, dtype=H, device="cuda")
    out = xv if stage_b else ov
    E.step_sde_stage(xv, bv, out, dv, None, m, m, 1.0, (1.5, 0.25, 0.0, 0.0, c1, c2, 1.0), terms, False, seeds=seeds, draw1=draw1,
                     draw2=draw2, noise1=noise1, noise2=noise2)
    torch.cuda.synchronize()
    n = B * row
    assert _tail_ok(xb, n) and _tail_ok(bb, n) and _tail_ok(ob, n) and _tail_ok(db, n) and bool((dv == 0).all())
    return out.cpu()


@pytest.mark.parametrize("B,row", [(1, 4), (3, 4 * 257), (1, BIG)])
def test_in_register_noise_equals_the_fill_of_stream_3(E, B, row):
    seeds = SEEDS[:B]
    fill = lambda draw, stream=3: E.philox_normal(torch.full((B, row), NAN, device="cuda"), seeds, draw, stream)  # noqa: E731
    f4, f5 = fill(4), fill(5)
    a_n1 = _noise_only(E, B, row, seeds, 4, 5, S.TERM_N1)
    assert torch.equal(a_n1, f4.cpu())                                   # stage A's n1 IS the fill of (draw1, stream 3)
    b_n1 = _noise_only(E, B, row, seeds, 4, 5, S.TERM_N1, stage_b=True)
    assert torch.equal(b_n1, a_n1)                                       # stage B's n1 is stage A's n1, bit for bit
    b_n2 = _noise_only(E, B, row, seeds, 4, 5, S.TERM_N2, stage_b=True)
    assert torch.equal(b_n2, f5.cpu()) and not torch.equal(b_n2, b_n1)   # and n2 the fill of (draw2, stream 3)
    # both terms with a real row's coefficients: drawn == fed, bit for bit, whichever of the two tensors is given
    _, _, _, _, c1, c2, _ = _row(2, "B", False).coef
    both = S.TERM_N1 | S.TERM_N2
    drawn = _noise_only(E, B, row, seeds, 4, 5, both, c1, c2, stage_b=True)
    for kw in (dict(noise1=f4, noise2=f5), dict(noise1=f4), dict(noise2=f5)):
        fed = _noise_only(E, B, row, seeds if len(kw) == 1 else None, 4, 5, both, c1, c2, stage_b=True, **kw)
        assert torch.equal(fed, drawn), list(kw)
    w = torch.tensor(c1) * f4.cpu() + torch.tensor(c2) * f5.cpu()        # fl(fl(0 + fl(c_1 n1)) + fl(c_2 n2))
    assert torch.equal(drawn, w)
    for other in (0, 1, 2):                                              # the other streams are other noise
        assert not torch.equal(fill(4, other).cpu(), a_n1)
    assert not torch.equal(_noise_only(E, B, row, seeds, 6, 5, S.TERM_N1), a_n1)


def test_the_two_stages_draw_increments_of_one_path(E):
    """x = 0, m = 0 and the rows of a real step at eta = 1: out_A / su1 = n1 and out_B / su2 = nB.  Their sample correlation over
    n = 65536 elements lies within five standard errors of a sample correlation, 5 (1 - rho^2) / sqrt(n), of
    rho = sqrt(d1 / (d1 + d2)); with two fresh draws in stage B it lies within 5 / sqrt(n) of 0."""
    n = 65536
    sig = [float(v) for v in _sigmas()]
    i = 2
    a, b = _row(i, "A", False), _row(i, "B", False)
    mid = math.sqrt(sig[i] * sig[i + 1])
    d1, d2 = sig[i] - mid, mid - sig[i + 1]
    rho = math.sqrt(d1 / (d1 + d2))
    _, su1 = S.get_ancestral_step(sig[i], mid, 1.0)
    _, su2 = S.get_ancestral_step(sig[i], sig[i + 1], 1.0)
    assert a.terms & 12 == S.TERM_N1 and b.terms & 12 == 12
    seeds = [4242]
    out_a = _noise_only(E, 1, n, seeds, 2 * i, 2 * i + 1, S.TERM_N1, a.coef[4], a.coef[5]).double().numpy().ravel() / su1
    out_b = _noise_only(E, 1, n, seeds, 2 * i, 2 * i + 1, 12, b.coef[4], b.coef[5], stage_b=True).double().numpy().ravel() / su2
    fresh = _noise_only(E, 1, n, seeds, 2 * i + 2, 2 * i + 3, 12, b.coef[4], b.coef[5], stage_b=True).double().numpy().ravel() / su2
    r = float(np.corrcoef(out_a, out_b)[0, 1])
    r0 = float(np.corrcoef(out_a, fresh)[0, 1])
    print(f"rho {rho:.6f}: sample correlation {r:.6f} (bound {5 * (1 - rho * rho) / math.sqrt(n):.2e}); fresh draws {r0:.6f}")
    assert abs(r - rho) <= 5 * (1 - rho * rho) / math.sqrt(n), (r, rho)
    assert abs(r0) <= 5 / math.sqrt(n), r0
    for v in (out_a, out_b):                                             # unit variance each: 5 standard errors sqrt(2 / n) of a variance
        assert abs(float(v.var()) - 1.0) <= 5 * math.sqrt(2.0 / n), float(v.var())


def test_more_chains_than_one_launch_carries_keys_for(E):
    """B = 33: the second launch's row is keyed by its own seed - chain 32 equals that seed run alone, and so does chain 5"""
    B, row = 33, 8
    r = _row(2, "B", True)
    seeds = list(range(100, 133))
    x, base, m_uc, m_c = _rand((B, row), 1, 3.0), _rand((B, row), 2, 3.0), _rand((B, row), 3, dtype=H), _rand((B, row), 4, dtype=H)

    def run(sl):
        xb, xv = _guarded(x[sl])
        bb, bv = _guarded(base[sl])
        cb, cv = _guarded(torch.full(x[sl].shape, NAN, dtype=H))
        E.step_sde_stage(xv, bv, xv, bv, cv, m_uc[sl].cuda(), m_c[sl].cuda(), 0.6, r.coef, r.terms, False, seeds=seeds[sl], draw1=4, draw2=5)
        torch.cuda.synchronize()
        n = xv.numel()
        assert _tail_ok(xb, n) and _tail_ok(bb, n) and _tail_ok(cb, n)
        return bv.cpu(), xv.cpu(), cv.cpu()
    big = run(slice(0, B))
    for b in (5, 32):
        one = run(slice(b, b + 1))
        assert all(torch.equal(u[b], v[0]) for u, v in zip(big, one)), b
    # den does not depend on the noise: bit for bit the model's; out with the model's noise within the generator's bound (tests/
    # test_gpu_sde_step.py: 8.5 * 2^-24 * 5.78 per normal with the model's own rounding) times |c_1| + |c_2|, plus one ulp of out for
    # each of the three roundings that may then fall the other way
    w = S.stage(x, base, m_uc, m_c, 0.6, r.coef, r.terms, False, S.noise_rows(B, row, seeds, 4), S.noise_rows(B, row, seeds, 5))
    assert torch.equal(big[0], w[0])
    tol = (abs(r.coef[4]) + abs(r.coef[5])) * 8.5 * 2.0 ** -24 * 5.78 + 3 * 2.0 ** -23 * float(w[1].abs().max())
    assert float((big[1] - w[1]).abs().max()) <= tol


def test_library_refusals_by_name(E):
    from cfgpp_amd import _lib
    from cfgpp_amd._lib import CfgppError
    lib = _lib.load()
    x, x2, out, den = (torch.zeros(2, 8, device="cuda") for _ in range(4))
    xc = torch.zeros(2, 8, dtype=H, device="cuda")
    m = torch.zeros(2, 8, dtype=H, device="cuda")
    ok = (1.0, 0.5, 0.5, 0.0, 0.3, 0.2, 1.0)
    arr = lambda c: (C.c_float * 7)(*c)  # noqa: E731
    seeds = (C.c_ulonglong * 2)(1, 2)

    def call(x_=x, base_=x, out_=out, den_=den, xc_=xc, uc_=m, c_=m, lam=1.0, coef=ok, terms=13, last=0, n1=None, n2=None, sd=seeds, B=2,
             row=8):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _lib.check(lib.cfgpp_step_sde_stage(p(x_), p(base_), p(out_), p(den_), p(xc_), p(uc_), p(c_), lam, None if coef is None else arr(coef),
                                            terms, last, p(n1), p(n2), sd, B, row, 0, 1, None), "cfgpp_step_sde_stage")
    call()                                                               # the plain call is fine
    call(base_=x2, out_=x, den_=x2)                                      # and so is the solver's stage B
    call(out_=x)                                                         # and a stage in place on x = base
    for kw in (dict(x_=None), dict(base_=None), dict(out_=None), dict(den_=None), dict(uc_=None), dict(c_=None), dict(coef=None)):
        with pytest.raises(CfgppError, match="cfgpp_step_sde_stage: null pointer"):
            call(**kw)
    with pytest.raises(CfgppError, match="out must not be base when base is not x"):
        call(base_=x2, out_=x2)
    with pytest.raises(CfgppError, match="den_out must not be x"):
        call(den_=x)
    with pytest.raises(CfgppError, match="den_out must not be out"):
        call(den_=out)
    with pytest.raises(CfgppError, match="B=0"):
        call(B=0)
    for row in (6, 0):
        with pytest.raises(CfgppError, match=f"row_elems={row}"):
            call(row=row)
    for t in (-1, 16):
        with pytest.raises(CfgppError, match=f"terms={t}"):
            call(terms=t)
    for j in range(7):
        for v in (NAN, float("inf")):
            c = list(ok)
            c[j] = v
            with pytest.raises(CfgppError, match=f"coef\\[{j}\\] is not finite"):
                call(coef=c)
    with pytest.raises(CfgppError, match="lam is not finite"):
        call(lam=NAN)
    for kw in (dict(), dict(n1=x2), dict(n2=x2), dict(terms=4), dict(terms=8)):
        with pytest.raises(CfgppError, match="a noise term needs its noise tensor or seeds_host"):
            call(sd=None, **kw)
    call(sd=None, last=1)                                                # the last step, a row without a noise term and fed noise need none
    call(sd=None, terms=3)
    call(sd=None, n1=x2, n2=x2)
    call(sd=None, terms=4, n1=x2)
    # and the Python wrapper refuses what never reaches the library
    with pytest.raises(CfgppError, match="a noise term needs seeds or its noise tensor"):
        E.step_sde_stage(x, x, out, den, xc, m, m, 1.0, ok, 13, False)
    with pytest.raises(CfgppError, match="3 seeds for 2 chains"):
        E.step_sde_stage(x, x, out, den, xc, m, m, 1.0, ok, 13, False, seeds=[1, 2, 3])
    with pytest.raises(CfgppError, match="must be fp32"):
        E.step_sde_stage(x.half(), x, out, den, xc, m, m, 1.0, ok, 13, False, seeds=[1, 2])
    with pytest.raises(CfgppError, match="size mismatch \\(den_out\\)"):
        E.step_sde_stage(x, x, out, den[:1], xc, m, m, 1.0, ok, 13, False, seeds=[1, 2])
    with pytest.raises(CfgppError, match="coef7"):
        E.step_sde_stage(x, x, out, den, xc, m, m, 1.0, ok + (0.0,), 13, False, seeds=[1, 2])
