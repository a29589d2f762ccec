"""-m gpu: the SDE kernels (include/cfgpp_sde.h; csrc/sde_kernels.hip) - cfgpp_step_sde and cfgpp_sde_input bit for bit against torch
evaluating the header's expression sequence (tests/sde_ref.py: step_sde) on torch-CPU and on torch-ROCm, the in-register noise
against cfgpp_philox_normal's fill (stream 2), chain independence past the 32 keys of one launch, and the library's refusals.

Like tests/test_gpu_lcm_step.py every output carries guard elements that must stay untouched, outputs are NaN-filled before the call,
every tensor the step must NOT read (history beyond n_hist, the noise of a step without a noise term, outputs) holds NaN, so a term
that is evaluated although it is skipped shows as a NaN; torch-ROCm is asked on tensors padded to whole 4096-element blocks (see
tests/test_gpu_vpred.py's docstring).  Coefficients are those of real steps - the first, a middle and the next-to-last step of a
6-step Karras schedule at eta = 1 - so the magnitudes are the product's."""
import ctypes as C
import math

import pytest
import torch

import sde_ref as S

pytestmark = pytest.mark.gpu

H, F = torch.float16, torch.float32
GUARD = 64
SENTINEL = 1234.0
NAN = float("nan")
SEEDS = [0x0123456789ABCDEF, 7, (1 << 63) + 12345]


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


def _coef(i, kind, cfgpp, n_hist, eta=1.0, solver_type="midpoint"):
    from cfgpp_amd.sde import sde_coeffs
    return sde_coeffs(_sigmas(), i, kind, solver_type, eta, 1.0, cfgpp, n_hist)


# (step of the 6-step schedule, kind, n_hist): first / middle / next to last step, every history depth each allows
STEPS = [(0, "2m", 0), (2, "2m", 1), (2, "3m", 1), (2, "3m", 0), (4, "3m", 2), (4, "2m", 1), (4, "3m", 0)]


def _options():
    out = []
    for i, kind, nh in STEPS:
        for cfgpp in (False, True):
            out.append(dict(i=i, kind=kind, n_hist=nh, cfgpp=cfgpp))
    out.append(dict(i=2, kind="2m", n_hist=1, cfgpp=False, solver_type="heun"))
    for cfgpp in (False, True):
        out.append(dict(i=4, kind="3m", n_hist=2, cfgpp=cfgpp, last=True))
        out.append(dict(i=4, kind="3m", n_hist=2, cfgpp=cfgpp, eta=0.0))                          # a_n = 0
        out.append(dict(i=4, kind="3m", n_hist=2, cfgpp=cfgpp, alias="hist2"))
        out.append(dict(i=2, kind="2m", n_hist=1, cfgpp=cfgpp, alias="hist1"))
        out.append(dict(i=4, kind="3m", n_hist=2, cfgpp=cfgpp, no_outs=True))
        out.append(dict(i=2, kind="3m", n_hist=1, cfgpp=cfgpp, single=True))
    out.append(dict(i=5, kind="3m", n_hist=2, cfgpp=True, last=True, no_outs=True))               # the schedule's own last step: zeros
    return out


def _run_case(E, B, row, o, k):
    cfgpp, nh, last = o["cfgpp"], o["n_hist"], bool(o.get("last"))
    coef = list(_coef(o["i"], o["kind"], cfgpp, nh, o.get("eta", 1.0), o.get("solver_type", "midpoint")))
    # what a skipped term leaves unused is finite and wrong on purpose: it must play no part
    if not cfgpp:
        coef[3] = 3.0
    if nh < 1:
        coef[4] = -2.0
    if nh < 2:
        coef[5] = 5.0
    noisy = not last and coef[6] != 0.0
    lam = 0.6 if cfgpp else 7.5
    seed = 1000 * k + row % 97 + B
    x = _rand((B, row), seed, float(coef[0]) if coef[0] > 1 else 1.3)
    m_uc = _rand((B, row), seed + 1, dtype=H)
    m_c = m_uc if o.get("single") else _rand((B, row), seed + 2, dtype=H)
    h1 = _rand((B, row), seed + 3, 1.1) if nh >= 1 else torch.full((B, row), NAN)
    h2 = _rand((B, row), seed + 4, 1.1) if nh == 2 else torch.full((B, row), NAN)
    noise = _rand((B, row), seed + 5) if noisy else torch.full((B, row), NAN)
    single = bool(o.get("single"))
    ref = lambda a, b, c, d, e, f_: S.step_sde(a, b, c, d, d if single else e, lam, coef, cfgpp, nh, last, f_, single=single)  # noqa: E731
    w = ref(x, h1, h2, m_uc, m_c, noise)                                                     # torch-CPU
    g = _on_rocm(ref, x, h1, h2, m_uc, m_c, noise)                                           # torch-ROCm
    n = B * row
    xb, xv = _guarded(x)
    db, dv = _guarded(torch.full((B, row), NAN))
    cb, cv = _guarded(torch.full((B, row), NAN, dtype=H))
    ub, uv = _guarded(m_uc, NAN)
    mb, mv = (ub, uv) if single else _guarded(m_c, NAN)
    h1b, h1v = _guarded(h1, NAN)
    h2b, h2v = _guarded(h2, NAN)
    nb, nv = _guarded(noise, NAN)
    ob, ov = _guarded(torch.full((B, row), NAN))
    alias = o.get("alias")
    hist_out = None if o.get("no_outs") else (h2v if alias == "hist2" else h1v if alias == "hist1" else ov)
    xc_out = None if o.get("no_outs") else cv
    E.step_sde(xv, dv, xc_out, h1v, h2v, hist_out, uv, mv, lam, coef, cfgpp, nh, last, noise=nv if noisy else None,
               seeds=None, draw=0)
    torch.cuda.synchronize()
    got = [dv.cpu(), None if hist_out is None else hist_out.cpu(), xv.cpu(), None if xc_out is None else cv.cpu()]
    bad = []
    for name, r in (("cpu", w), ("rocm", g)):
        for what, a, b in zip(("den", "hist", "x", "xc"), got, r):
            if a is None:
                continue
            assert bool(torch.isfinite(a.float()).all()), (what, o)
            d = int((a.flatten() != b.flatten().to(a.dtype)).sum()) if a.dtype == b.dtype else -1
            if d:
                bad.append((name, what, d))
    if last:
        assert torch.equal(got[0], got[2])                              # x' = den
    if not cfgpp and got[1] is not None:
        assert torch.equal(got[1], got[0])                              # CFG: the history holds den
    # guards: nothing is written past the end of any buffer, inputs are left alone, unused outputs stay NaN
    for buf, fill in ((xb, SENTINEL), (db, SENTINEL), (cb, SENTINEL), (ob, SENTINEL), (ub, NAN), (mb, NAN), (h1b, NAN), (h2b, NAN), (nb, NAN)):
        assert _tail_ok(buf, n, fill), o
    assert torch.equal(uv.cpu(), m_uc) and (noisy is False or torch.equal(nv.cpu(), noise))
    if alias != "hist1" and nh >= 1:
        assert torch.equal(h1v.cpu(), h1)
    if alias is not None or o.get("no_outs"):
        assert bool(torch.isnan(ov.cpu()).all())
    if o.get("no_outs"):
        assert bool(torch.isnan(cv.float().cpu()).all())
    return bad


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("row", [4, 1020, 1024, 4100])
def test_step_sde_equals_torch_bit_for_bit(E, B, row):
    bad = []
    for k, o in enumerate(_options()):
        for item in _run_case(E, B, row, o, k):
            bad.append((o, item))
    assert not bad, bad[:6]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("row", [4, 1020, 1024, 4100])
def test_sde_input_equals_torch_bit_for_bit(E, B, row):
    from cfgpp_amd.sde import input_scale
    for j, sigma in enumerate((14.6146, 1.2741, 0.1303)):
        s_in = input_scale(sigma)
        x = _rand((B, row), 50 + j + row, sigma if sigma > 1 else 1.0)
        fn = lambda a: ((a * torch.tensor(s_in, dtype=F, device=a.device)).to(H),)  # noqa: E731
        w, g = fn(x)[0], _on_rocm(fn, x)[0]
        xb, xv = _guarded(x)
        cb, cv = _guarded(torch.full((B, row), NAN, dtype=H))
        E.sde_input(xv, cv, s_in)
        torch.cuda.synchronize()
        got = cv.cpu()
        assert torch.equal(got.flatten(), w.flatten()) and torch.equal(got.flatten(), g)
        assert _tail_ok(xb, B * row) and _tail_ok(cb, B * row) and torch.equal(xv.cpu(), x)


def test_sde_input_odd_sizes(E):
    """cfgpp_sde_input takes any n >= 1: whole groups by vector accesses, the up-to-3 trailing elements one by one"""
    for n in (1, 2, 3, 5, 1023, 1026, 4099):
        x = _rand((1, n), n, 2.0)
        xb, xv = _guarded(x)
        cb, cv = _guarded(torch.full((1, n), NAN, dtype=H))
        E.sde_input(xv, cv, 0.37)
        torch.cuda.synchronize()
        assert torch.equal(cv.cpu(), (x * torch.tensor(0.37, dtype=F)).to(H)) and _tail_ok(cb, n) and _tail_ok(xb, n)


def _step_with(E, B, row, seeds, draw, noise, coef, x, m_uc, m_c, h1):
    xb, xv = _guarded(x)
    db, dv = _guarded(torch.full((B, row), NAN))
    cb, cv = _guarded(torch.full((B, row), NAN, dtype=H))
    ob, ov = _guarded(torch.full((B, row), NAN))
    E.step_sde(xv, dv, cv, h1.cuda(), None, ov, m_uc.cuda(), m_c.cuda(), 0.6, coef, True, 1, False, seeds=seeds, draw=draw,
               noise=None if noise is None else noise.cuda())
    torch.cuda.synchronize()
    n = B * row
    assert _tail_ok(xb, n) and _tail_ok(db, n) and _tail_ok(cb, n) and _tail_ok(ob, n)
    return dv.cpu(), ov.cpu(), xv.cpu(), cv.cpu()


@pytest.mark.parametrize("B,row", [(1, 4), (3, 1020), (3, 1024), (1, 4100), (3, 4100)])
def test_in_register_noise_equals_the_fill_of_stream_2(E, B, row):
    coef = _coef(2, "2m", True, 1)
    seeds = SEEDS[:B]
    x, m_uc, m_c, h1 = _rand((B, row), 5 + row, 3.0), _rand((B, row), 6, dtype=H), _rand((B, row), 7, dtype=H), _rand((B, row), 8)
    fill = lambda stream: E.philox_normal(torch.full((B, row), NAN, device="cuda"), seeds, 3, stream).cpu()  # noqa: E731
    drawn = _step_with(E, B, row, seeds, 3, None, coef, x, m_uc, m_c, h1)
    fed = _step_with(E, B, row, None, 0, fill(2), coef, x, m_uc, m_c, h1)
    assert all(torch.equal(a, b) for a, b in zip(drawn, fed))
    for other in (0, 1):                                                # streams 0 (LCM) and 1 (ancestral) are other noise
        alt = _step_with(E, B, row, None, 0, fill(other), coef, x, m_uc, m_c, h1)
        assert torch.equal(alt[0], drawn[0]) and not torch.equal(alt[2], drawn[2])
    nxt = _step_with(E, B, row, seeds, 4, None, coef, x, m_uc, m_c, h1)      # another draw index: another x, the same den
    assert torch.equal(nxt[0], drawn[0]) and torch.equal(nxt[1], drawn[1]) and not torch.equal(nxt[2], drawn[2])
    # and the drawn noise is the float64 Philox model's: (x' - x' without the noise term) / a_n = noise, up to the two roundings of
    # fl(acc + fl(a_n n)) (half an ulp of a_n n <= 2^-24 * 5.78 a_n, half an ulp of x' <= 2^-24 |x'|), the generator's own bound
    # (tests/test_gpu_lcm_step.py: 8 * 2^-24 |n| + 2^-40, |n| <= 5.78) and the model's rounding to fp32 (2^-25 * 5.78)
    quiet = list(coef)
    quiet[6] = 0.0
    base = _step_with(E, B, row, None, 0, None, quiet, x, m_uc, m_c, h1)
    model = S.noise_rows(B, row, seeds, 3)
    err = ((drawn[2].double() - base[2].double()) / coef[6] - model.double()).abs().max()
    bound = 2.0 ** -24 * (5.78 + float(drawn[2].abs().max()) / coef[6]) + (8.5 * 2.0 ** -24) * 5.78 + 2.0 ** -40
    assert float(err) <= bound, (float(err), bound)


def test_more_chains_than_one_launch_carries_keys_for(E):
    """B = 35: the second launch's rows are keyed by their own seeds - row 33 equals that seed run alone"""
    B, row = 35, 8
    coef = _coef(2, "2m", True, 1)
    seeds = list(range(100, 135))
    x, m_uc, m_c, h1 = _rand((B, row), 1, 3.0), _rand((B, row), 2, dtype=H), _rand((B, row), 3, dtype=H), _rand((B, row), 4)
    big = _step_with(E, B, row, seeds, 1, None, coef, x, m_uc, m_c, h1)
    one = _step_with(E, 1, row, seeds[33:34], 1, None, coef, x[33:34], m_uc[33:34], m_c[33:34], h1[33:34])
    assert all(torch.equal(a[33], b[0]) for a, b in zip(big, one))
    w = S.step_sde(x, h1, None, m_uc, m_c, 0.6, coef, True, 1, False, S.noise_rows(B, row, seeds, 1))
    assert torch.equal(big[0], w[0]) and torch.equal(big[1], w[1])      # den / history do not depend on the noise: bit for bit
    # x': the model's noise within the generator's bound (8.5 * 2^-24 * 5.78 with the model's own rounding), times a_n, plus one ulp of
    # x' for each of the two roundings that may then fall the other way
    tol = coef[6] * 8.5 * 2.0 ** -24 * 5.78 + 2 * 2.0 ** -23 * float(w[2].abs().max())
    assert float((big[2] - w[2]).abs().max()) <= tol


def test_library_refusals_by_name(E):
    from cfgpp_amd import _lib
    from cfgpp_amd._lib import CfgppError
    lib = _lib.load()
    x, den, h1 = (torch.zeros(2, 8, device="cuda") for _ in range(3))
    xc = torch.zeros(2, 8, dtype=H, device="cuda")
    m = torch.zeros(2, 8, dtype=H, device="cuda")
    ok = (1.0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.3, 1.0)
    arr = lambda c: (C.c_float * 8)(*c)  # noqa: E731
    seeds = (C.c_ulonglong * 2)(1, 2)

    def call(x_=x, den_=den, xc_=xc, h1_=None, h2_=None, ho_=None, uc_=m, c_=m, lam=1.0, coef=ok, cfgpp=0, n_hist=0, last=0, noise=None,
             sd=seeds, B=2, row=8):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _lib.check(lib.cfgpp_step_sde(p(x_), p(den_), p(xc_), p(h1_), p(h2_), p(ho_), p(uc_), p(c_), lam, None if coef is None else arr(coef),
                                      cfgpp, n_hist, last, p(noise), sd, B, row, 0, None), "cfgpp_step_sde")
    call()                                                               # the plain call is fine
    for kw in (dict(x_=None), dict(den_=None), dict(uc_=None), dict(c_=None), dict(coef=None)):
        with pytest.raises(CfgppError, match="cfgpp_step_sde: null pointer"):
            call(**kw)
    with pytest.raises(CfgppError, match="den_out must not be x"):
        call(den_=x)
    with pytest.raises(CfgppError, match="B=0"):
        call(B=0)
    for row in (6, 0):
        with pytest.raises(CfgppError, match=f"row_elems={row}"):
            call(row=row)
    for nh in (-1, 3):
        with pytest.raises(CfgppError, match=f"n_hist={nh}"):
            call(n_hist=nh)
    with pytest.raises(CfgppError, match="n_hist=1 needs hist1"):
        call(n_hist=1)
    with pytest.raises(CfgppError, match="n_hist=2 needs hist2"):
        call(n_hist=2, h1_=h1)
    for j in (0, 3, 6, 7):
        for v in (NAN, float("inf")):
            c = list(ok)
            c[j] = v
            with pytest.raises(CfgppError, match=f"coef\\[{j}\\] is not finite"):
                call(coef=c)
    with pytest.raises(CfgppError, match="lam is not finite"):
        call(lam=NAN)
    with pytest.raises(CfgppError, match="needs noise or seeds_host"):
        call(sd=None)
    call(sd=None, last=1)                                                # the last step and a step without a noise term need neither
    call(sd=None, coef=ok[:6] + (0.0, 1.0))
    with pytest.raises(CfgppError, match="cfgpp_sde_input: null pointer"):
        _lib.check(lib.cfgpp_sde_input(None, xc.data_ptr(), 1.0, 16, None), "cfgpp_sde_input")
    with pytest.raises(CfgppError, match="cfgpp_sde_input: n=0"):
        _lib.check(lib.cfgpp_sde_input(x.data_ptr(), xc.data_ptr(), 1.0, 0, None), "cfgpp_sde_input")
    with pytest.raises(CfgppError, match="s_in is not finite"):
        _lib.check(lib.cfgpp_sde_input(x.data_ptr(), xc.data_ptr(), NAN, 16, None), "cfgpp_sde_input")
    # and the Python wrappers refuse what never reaches the library
    with pytest.raises(CfgppError, match="needs seeds or noise"):
        E.step_sde(x, den, xc, None, None, None, m, m, 1.0, ok, False, 0, False)
    with pytest.raises(CfgppError, match="3 seeds for 2 chains"):
        E.step_sde(x, den, xc, None, None, None, m, m, 1.0, ok, False, 0, False, seeds=[1, 2, 3])
    with pytest.raises(CfgppError, match="must be fp32"):
        E.step_sde(x.half(), den, xc, None, None, None, m, m, 1.0, ok, False, 0, False, seeds=[1, 2])
    with pytest.raises(CfgppError, match="size mismatch"):
        E.step_sde(x, den[:1], xc, None, None, None, m, m, 1.0, ok, False, 0, False, seeds=[1, 2])
    with pytest.raises(CfgppError, match="x must be fp32 and xc_out fp16"):
        E.sde_input(x, den, 1.0)
