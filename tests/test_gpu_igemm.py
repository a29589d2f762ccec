"""-m gpu: every dispatch path of the implicit-GEMM launcher (csrc/igemm_kernel.hip, big4_kernel.hip, big4p_kernel.hip) against the
fp64 references of tests/igemm_cases.py, per element.

Every case is launched twice into guarded destinations: 4096 sentinel elements before and after; the interior NaN (an element the
kernel never stores stays NaN); the halo of a padded destination holds the sentinel and must not be touched; head-major
destinations are zero, as the engines allocate them, with NaN in the live region, and their pads must still be zero.  Source halos
are zero.  Then:
  * cfgpp_igemm_last_launch equals igemm_cases.expected_launch(case) after both launches - the kernel instance, tile walk, K-split
    and epilogue variant the case is named after really ran (and cfgpp_igemm_last_config_ran agrees);
  * guards, halo and pads intact, the live region finite everywhere, the second launch bit-identical;
  * per element |got - ref64| <= igemm_cases.bound (derived, see there), and the whole-tensor rel-L2 < 1.5e-3 of the older tests;
  * the bit-identity the launcher claims: within a shape every whole-tile launch except the 16x16x32-MFMA tile (configs 18 / 19: another
    k order) gives the same bits, whatever tile, ring depth, staging, walk or epilogue variant ran.  One exception is arithmetic, not
    order: with a residual, the LDS-staged store epilogues round to fp16 before the residual is added (torch's fp16 `conv + residual`)
    and the generic epilogue adds it in fp32, so the two variants are compared among themselves.  K-split launches are held to the
    bound only.
tests/test_igemm_cases_cpu.py shows which faults these conditions catch.

Worst err / bound per group on the MI355X (434 cases, every one with the predicted report): tiles_store 0.982, tiles_fallback 0.948,
amodes 0.949, epilogues_generic 0.925, epilogues_staged 0.952, staging 0.904, ksplit 0.752, walks 0.917, heuristic 0.948 - the
figures of the fp32 model on the CPU, to three digits; largest rel-L2 2.8e-4."""
import numpy as np
import pytest
import torch

import igemm_cases as IC
from test_gpu_configs import need_gpu, record

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = -1234.0
ids = dict(ids=lambda c: c.id)

_DEV = {}          # Problem -> device tensors of its inputs
_BITS = {}         # (Problem, epilogue class) -> (case id, the bits of the first whole-tile launch on that shape)


def _dev(p):
    import hip_ops as H
    if p not in _DEV:
        d = IC.device_buffers(p)

        def up(a):
            return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(H.DEV)
        _DEV[p] = dict(src=[up(s) for s in d.src], w=up(d.w), bias=up(d.bias), temb=up(d.temb), resid=up(d.resid))
    return _DEV[p]


def _guarded(shape, fill, dtype=torch.float16):
    import hip_ops as H
    n = int(np.prod(shape))
    buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=dtype, device=H.DEV)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return buf, view


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _set_switches(lib, c):
    lib.cfgpp_igemm_force_config(c.cfg)
    lib.cfgpp_igemm_force_split(c.split)
    lib.cfgpp_igemm_set_staging(c.staging)
    lib.cfgpp_igemm_set_staged_epilogue(c.staged_epi)
    lib.cfgpp_igemm_set_n_major(c.n_major)
    lib.cfgpp_igemm_set_blocked_walk(c.blocked)
    lib.cfgpp_igemm_set_tail_split(c.tail_split)


def _restore_switches(lib):
    lib.cfgpp_igemm_force_config(0)
    lib.cfgpp_igemm_force_split(0)
    lib.cfgpp_igemm_set_staging(1)
    lib.cfgpp_igemm_set_staged_epilogue(1)
    lib.cfgpp_igemm_set_n_major(-1)
    lib.cfgpp_igemm_set_blocked_walk(1)
    lib.cfgpp_igemm_set_tail_split(1)
    lib.cfgpp_op_igemm_set_gstat(None)


def _launch_once(lib, c):
    """one guarded launch -> (list of (whole buffer, written view), [rows, n_out] of what was stored as fp64 numpy, problems)"""
    import hip_ops as H
    p, d = c.p, _dev(c.p)
    problems, bufs = [], []
    if p.op == "heads":
        lay = IC.heads_layout(p)
        flat = {}
        for part in lay.parts:
            buf, v = _guarded(lay.shapes[part], 0.0)
            live = torch.from_numpy(np.unique(lay.off[lay.part == part])).to(H.DEV)
            v.view(-1)[live] = float("nan")
            bufs.append((buf, v))
            flat[part] = (v, live)
        ptr = {part: H.P(flat[part][0]) if part in flat else None for part in (0, 1, 2)}
        qp, kp = lay.shapes[0][1], lay.shapes[1][1]
        H.check(lib.cfgpp_op_igemm_heads_ex(H.P(d["src"][0]), p.K, H.P(d["w"]), p.rows, p.N, H.P(d["bias"]), p.tokens, ptr[0], ptr[1], ptr[2],
                                            p.part0, p.part_width, p.head_dim, p.nheads, qp, kp, p.vt_linear, H.stream()), "cfgpp_op_igemm_heads_ex")
        report = H.igemm_last_launch()
        torch.cuda.synchronize()
        got = np.empty((p.rows, p.N))
        for part in lay.parts:
            v, live = flat[part]
            host = v.view(-1).double().cpu().numpy()
            sel = lay.part == part
            got[sel] = host[lay.off[sel]]
            pads = host.copy()
            pads[live.cpu().numpy()] = 0.0
            if np.any(pads != 0.0) or not np.isfinite(pads).all():
                problems.append(f"pads of the part-{part} buffer are no longer zero")
        return bufs, got, report, problems
    shape = (p.B, p.H + 2, p.W + 2, p.n_out) if p.padded else (p.rows, p.n_out)
    buf, o = _guarded(shape, SENTINEL)
    inner = o[:, 1:-1, 1:-1] if p.padded else o
    inner.fill_(float("nan"))
    bufs.append((buf, o))
    if c.gstat:
        gbuf, gv = _guarded((IC.cdiv(p.rows, 32) * p.N * 2,), float("nan"), dtype=torch.float32)
        bufs.append((gbuf, gv))
        lib.cfgpp_op_igemm_set_gstat(H.P(gv))
    a1 = d["src"][1] if len(d["src"]) > 1 else None
    H.igemm_ex(d["src"][0], a1, p.C0, p.C1, p.taps, p.amode, p.H, p.W, d["w"], p.rows, p.N, bias=d["bias"], temb=d["temb"], temb_ld=p.N,
               resid=d["resid"], rmode=1 if p.padded else 0, rld=p.N, out=o, omode=1 if p.padded else 0, old=p.n_out, epi=p.epi,
               ashift=p.ashift, out_scale=p.out_scale, cfg_hint=c.hint)
    report = H.igemm_last_launch()
    wrote = int(lib.cfgpp_op_igemm_gstat_written())
    torch.cuda.synchronize()
    if wrote != report[12]:
        problems.append(f"stat_flag says {wrote}, the report {report[12]}")
    if c.gstat and report[12] and not bool(torch.isfinite(bufs[-1][1]).all()):
        problems.append("statistics reported as written, but slots are unwritten")
    if p.padded:
        halo = o.clone()
        halo[:, 1:-1, 1:-1] = SENTINEL
        if not bool((halo == SENTINEL).all()):
            problems.append("halo written")
    got = inner.reshape(p.rows, p.n_out).double().cpu().numpy()
    return bufs, got, report, problems


def run_case(c):
    need_gpu()
    import hip_ops as H
    lib = H.lib()
    want = IC.expected_launch(c)
    ref = IC.reference(c.p).ref
    try:
        _set_switches(lib, c)
        first = _launch_once(lib, c)
        ran = int(lib.cfgpp_igemm_last_config_ran())
        second = _launch_once(lib, c)
    except RuntimeError as e:
        # a device error (or a refusal the table should not hold): nothing more is launched on this GPU by this session
        pytest.exit(f"{c.id}: {e}", returncode=3)
    finally:
        _restore_switches(lib)
    bufs, got, report, problems = first
    problems = list(problems) + [f"second launch: {q}" for q in second[3]]
    for k, r in enumerate((report, second[2])):
        if r != want:
            diff = {IC.REPORT_FIELDS[i]: (r[i], want[i]) for i in range(16) if r[i] != want[i]}
            problems.append(f"launch {k + 1} reported (got, expected) {diff}")
    if ran != IC.expected_config_ran(c):
        problems.append(f"cfgpp_igemm_last_config_ran {ran}, expected {IC.expected_config_ran(c)}")
    if not all(_guards_intact(b) for b, _ in bufs + second[0]):
        problems.append("guard elements written")
    nonfinite = int((~np.isfinite(got)).sum())
    if nonfinite:
        problems.append(f"{nonfinite} output elements not finite (unwritten or NaN)")
    for (_, v1), (_, v2) in zip(bufs[:1] if c.p.op != "heads" else bufs, second[0]):
        if not torch.equal(v1.view(torch.int16), v2.view(torch.int16)):
            problems.append("second launch differs")
    g0 = np.nan_to_num(got)
    bnd = IC.bound(c, g0)
    ratio = float((np.abs(g0 - ref) / bnd).max()) if not nonfinite else float("inf")
    rel = IC.rel_l2(g0, ref)
    # the bits of every whole-tile launch on this shape (see the module docstring)
    if report[7] == 1 and report[0] != 3 and not nonfinite:
        key = (c.p, report[13] if (c.p.op == "store" and c.p.resid) else -1)
        bits = got.astype(np.float16).tobytes()
        if key not in _BITS:
            _BITS[key] = (c.id, bits)
        elif _BITS[key][1] != bits:
            problems.append(f"bits differ from {_BITS[key][0]} on the same shape")
    record("igemm_case", group=c.group, case=c.id, launch=list(report), ratio=ratio, rel_l2=rel, problems=problems)
    print(f"{c.id}: launch {report} err / bound {ratio:.3f} rel_l2 {rel:.3e} {problems}")
    assert not problems, (c.id, problems)
    assert ratio <= 1.0, f"{c.id}: |got - ref64| is {ratio:.3f} x the bound at its worst element"
    assert rel < IC.REL_L2_BOUND, f"{c.id}: rel-L2 {rel:.3e}"


def _param(group):
    return pytest.mark.parametrize("c", IC.GROUPS[group], **ids)


@_param("tiles_store")
def test_tiles_store(c):
    """every tile of launch_config: ragged M and N, 1 / 2 / stages / stages + 1 K-tiles, bias + residual; conv3x3 + temb across samples"""
    run_case(c)


@_param("tiles_fallback")
def test_tiles_fallback(c):
    """launches a forced config does not admit: the report names the tile that ran instead"""
    run_case(c)


@_param("amodes")
def test_amodes(c):
    """stride 2 with pad 1 and pad (0,1,0,1) on odd and even sources, fused upsample, two sources, token rows into a padded map"""
    run_case(c)


@_param("epilogues_generic")
def test_epilogues_generic(c):
    """the generic epilogue: staged forms switched off, N % 8 == 4, GEGLU at N % 128 != 0, heads at 77 tokens, out_scale"""
    run_case(c)


@_param("epilogues_staged")
def test_epilogues_staged(c):
    """the same operations at shapes that take the LDS-staged store / GEGLU / heads epilogues of every family"""
    run_case(c)


@_param("staging")
def test_register_staging(c):
    """configs 21 .. 23 and cfgpp_igemm_set_staging(0): the register-staged loader, parameters from global memory"""
    run_case(c)


@_param("ksplit")
def test_ksplit(c):
    """forced splits 2, 3 and one K-tile per slice, the tail rule at K = 2048 / 4096, and the tiles the rule leaves whole"""
    run_case(c)


@_param("walks")
def test_tile_walks(c):
    """M-major, N-major and the XCD-blocked 2-D walk over the same 64 tiles: the same bits"""
    run_case(c)


@_param("heuristic")
def test_heuristic_and_hints(c):
    """no forced config: the rule's small-problem branches, and cfg_hint valid / overridden by the K-split rule / invalid"""
    run_case(c)


def test_a_refused_launch_clears_the_report():
    need_gpu()
    import hip_ops as H
    lib = H.lib()
    c = IC.GROUPS["heuristic"][0]
    run_case(c)
    assert H.igemm_last_launch() == IC.expected_launch(c)
    d = _dev(c.p)
    out = torch.empty((c.p.rows, c.p.N), dtype=torch.float16, device=H.DEV)
    rc = lib.cfgpp_op_igemm_ex(H.P(d["src"][0]), None, c.p.C0, 0, 1, 0, 0, 0, H.P(d["w"]), c.p.rows, c.p.N + 2, None, None, 0, None, 0, 0,
                               H.P(out), 0, c.p.N, 0, 0, 1.0, 0, H.stream())            # N % 4 != 0: refused on the host
    assert rc != 0 and H.igemm_last_launch() == (0,) * 16
