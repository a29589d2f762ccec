"""CPU: the non-square and minimal latents of tests/geometry_cases.py do what they are there for, on the fp32 oracle alone.

    G1  the gap: at 16 x 16 every `pitch` fault changes nothing, exactly - no square test can see an H / W mix-up of this kind.
    G2  loudness: every site of every engine, both fault kinds, moves the oracle by >= 4 T in one of the engine's non-square cases.
    G3  room: the fp16-activation emulation stays within 0.6 T of the oracle at every tested t, for every case asserted at T.
    G4  the inventory: the sites of a case are the sites its config has, counted from the config.
    G5  the fault models on a hand-made 2 x 3 plane.
    and the deliberate check: the oracle with one `pitch` fault, compared with the honest oracle the way the GPU test compares an
    engine, fails at T for every site, and ``explain`` names the site.

T is the tolerance of the existing engine tests (loud_cases.T_UNET); nothing here was measured on an engine."""
import pytest
import torch

import geometry_cases as G
import loud_cases as L

ENGINES = {}
for _c in G.LOUD + G.FEATURES:
    ENGINES.setdefault(G.engine_key(_c), []).append(_c)
ENGINE_IDS = ["-".join(k) for k in ENGINES]


def test_the_case_table_holds_every_shape_it_is_there_for():
    ids = [G.case_id(c) for c in G.all_cases()]
    assert len(set(ids)) == len(ids)
    for want in ("tiny_sd-8x24", "tiny_sd-20x12", "tiny_xl-6x10", "tiny_xl-8x24", "tiny_sd2-8x12", "tiny_sd_inpaint-8x12", "tiny_sd_lcm-12x8",
                 "controlnet-tiny_sd-8x24", "controlnet-tiny_sd-20x12", "tiny_sd-12x4", "tiny_sd-4x12", "tiny_sd-4x4", "tiny_xl-2x6", "tiny_xl-2x2",
                 "controlnet-tiny_sd-12x4", "freeu-tiny_sd-8x24", "freeu-tiny_sd-20x12", "regions-tiny_sd-8x24", "regions-tiny_sd-20x12",
                 "tiny_sd_inpaint-8x24", "tiny_sd_inpaint-20x12"):
        assert want in ids, want
    assert G.T == L.T_UNET == 2.5e-3 and G.TS == (500.0, 981.0, 1.0) and G.R == 4 and G.ZR == 2
    from cfgpp_amd.unet_config import CONFIGS
    for c in G.all_cases():
        cfg = CONFIGS[c.cfg]
        f = 1 << (cfg.num_levels - 1)
        assert c.hw[0] % f == 0 and c.hw[1] % f == 0
        bottom = (c.hw[0] // f, c.hw[1] // f)
        if c in G.LOUD or c in G.FEATURES:        # an H / W fault must show at the deepest level too
            assert min(bottom) >= 2 and bottom[0] != bottom[1], (G.case_id(c), bottom)
        else:
            assert min(bottom) == 1, (G.case_id(c), bottom)
        e = G.engine(c)
        inp = e.inputs
        assert inp["z"].shape == (G.ZR, 4) + tuple(c.hw)
        assert not torch.equal(inp["z"][0], inp["z"][1])
        if c.engine != "regions":                 # context at scale 0.5 (the regions' contexts are region_ref's)
            assert inp["ehs"].shape[:2] == (G.R, 77) and 0.45 < float(inp["ehs"].std()) < 0.55
        if "ti" in inp:
            assert all(len(set(row.tolist())) == 6 for row in inp["ti"]) and not torch.equal(inp["ti"][0], inp["ti"][G.ZR])
        if "img" in inp:
            assert inp["img"].shape == (G.ZR, 3, 8 * c.hw[0], 8 * c.hw[1])
        # synth weights, the project's own, but for the one key of the "hint10" ControlNet
        want = L.synth_weights(cfg if c.engine != "controlnet" else ("controlnet", cfg), 0)
        other = [k for k in want if not torch.equal(want[k].float(), e.sd[k])]
        assert list(e.sd) == list(want)
        assert other == ([k for k in want if k.startswith(G.HINT_KEY)] if c.weights == "hint10" else []), (G.case_id(c), other)
    assert G.bound(G.all_cases()[0], 500.0) == G.T and G.RELAXED == ()


# ---------------------------------------------------------------------------------------------------------------- G5
def test_g5_the_fault_models_on_a_2_by_3_plane():
    x = torch.arange(6.0).reshape(1, 1, 2, 3)                    # [[0 1 2] [3 4 5]]
    # pitch H = 2 instead of W = 3: out[y, x] = flat[(2 y + x) mod 6]
    assert G.pitch(x).reshape(-1).tolist() == [0.0, 1.0, 2.0, 2.0, 3.0, 4.0]
    # x-major fill: the transposed plane [[0 3] [1 4] [2 5]] read as 2 x 3
    assert G.transpose(x).reshape(-1).tolist() == [0.0, 3.0, 1.0, 4.0, 2.0, 5.0]
    y = torch.arange(6.0).reshape(1, 1, 3, 2)                    # [[0 1] [2 3] [4 5]]: out[y, x] = flat[(3 y + x) mod 6]
    assert G.pitch(y).reshape(-1).tolist() == [0.0, 1.0, 3.0, 4.0, 0.0, 1.0]
    assert G.transpose(y).reshape(-1).tolist() == [0.0, 2.0, 4.0, 1.0, 3.0, 5.0]
    sq = torch.randn(2, 3, 4, 4)
    assert torch.equal(G.pitch(sq), sq) and torch.equal(G.transpose(sq), sq.transpose(-1, -2)) and not torch.equal(G.transpose(sq), sq)
    # both keep shape and memory layout, and act on every leading axis alike (an integer region map [rows, H, W] too)
    cl = torch.randn(2, 3, 2, 3).permute(0, 3, 1, 2)
    for fn in (G.pitch, G.transpose):
        assert fn(cl).shape == cl.shape and fn(cl).stride() == cl.stride() and torch.equal(fn(cl)[1, 2], fn(cl[1:2, 2:3])[0, 0])
        ids = torch.arange(12).reshape(2, 2, 3)
        assert fn(ids).dtype == torch.int64 and torch.equal(fn(ids)[1], fn(ids[1:])[0])


# ---------------------------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("case", G.SQUARE, ids=G.case_id)
def test_g1_no_pitch_fault_shows_on_a_square_latent(case):
    for s in G.sites(case):
        assert G.effect(case, s, "pitch") == 0.0, s
    # not because the sites do nothing: the other model, which does move a square plane, is loud at every one of them
    quiet = [(s, G.effect(case, s, "transpose")) for s in G.sites(case)[::5]]
    assert all(v >= 4 * G.T for _, v in quiet), quiet


# ---------------------------------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("key", list(ENGINES), ids=ENGINE_IDS)
def test_g2_every_site_is_loud_in_a_non_square_case(key, kind):
    need = 4 * G.T
    cases = ENGINES[key]
    all_sites = []
    for c in cases:
        all_sites += [s for s in G.sites(c) if s not in all_sites]
    quiet = []
    for s in all_sites:
        best = 0.0
        for c in cases:
            if s in G.sites(c):
                best = max(best, G.effect(c, s, kind))
                if best >= need:
                    break
        if best < need:
            quiet.append((s, best))
    assert not quiet, f"{key} {kind}: {len(quiet)} of {len(all_sites)} sites below 4 T = {need:g} in every case: {quiet}"


# ---------------------------------------------------------------------------------------------------------------- G3
@pytest.mark.parametrize("case", G.all_cases(), ids=G.case_id)
def test_g3_the_tolerance_leaves_room(case):
    for t in G.TS:
        em = G.emulated(case, t)
        print(f"{G.case_id(case)} t={t}: emulated {em:.3e} ({em / G.T:.2f} T), bound {G.bound(case, t):.3e}")
        assert G.bound(case, t) >= G.T
        if case not in G.RELAXED:
            assert em <= G.ROOM * G.T, (G.case_id(case), t, em)
            assert G.bound(case, t) == G.T
    if case != G.ONE_TOKEN:
        assert G.ENGINE_OVER_EMULATION * G.ROOM < 1.0
    for o in G.engine(case).base(G.TS[0]):
        assert torch.isfinite(o).all()


def test_g3_the_emulation_is_not_the_oracle():
    """it rounds: at 16 x 16 it stands where profiles/loud_weights/README.md puts the synth weights (1.0e-3; the MI355X 1.2e-3)"""
    em = G.emulated(G.SQUARE[0], 500.0)
    assert 0.8e-3 < em < 1.2e-3, em


# ---------------------------------------------------------------------------------------------------------------- G4
@pytest.mark.parametrize("case", G.all_cases() + G.SQUARE, ids=G.case_id)
def test_g4_the_sites_are_all_the_sites_of_the_config(case):
    sites = G.sites(case)
    assert len(set(sites)) == len(sites)
    got = {}
    for s in sites:
        got[G.site_group(s)] = got.get(G.site_group(s), 0) + 1
    want = {k: v for k, v in G.expected_sites(case).items() if v}
    assert got == want, (G.case_id(case), got, want)
    if case.engine == "unet" and case.cfg in ("tiny_sd", "tiny_xl"):
        assert len(sites) == {"tiny_sd": 26, "tiny_xl": 16}[case.cfg]


# ---------------------------------------------------------------------------------------------------------------- the deliberate check
@pytest.mark.parametrize("case", [G.LOUD[0], G.LOUD[2]], ids=G.case_id)
def test_a_planted_pitch_fault_fails_at_t_and_is_named(case):
    """the oracle with one pitch fault in the engine's place: the comparison of tests/test_gpu_geometry_engines.py fails at T for
    every site, and its failure message names the site first"""
    e = G.engine(case)
    t = 500.0
    for s in G.sites(case):
        got = [b + d for b, d in zip(e.base(t), G.change(case, s, "pitch", t))]
        rels = [L.rel_l2(g, b) for g, b in zip(got, e.base(t))]
        assert not all(r < G.bound(case, t) for r in rels), (s, rels)
        top = G.suspects(case, t, got)
        assert top.startswith(f"pitch: {s} (cos +1.00"), (s, top)


def test_an_honest_residual_accuses_no_site():
    """the emulation's own residual (rounding noise) is collinear with no spatial fault"""
    case, t = G.LOUD[0], 500.0
    e = G.engine(case)
    got = list(e.outputs(e.sd, dict(e.inputs, emulate=True), t))
    res = [g - b for g, b in zip(got, e.base(t))]
    assert all(abs(c) < 0.2 for _, c, _ in L.explain(res, G.fault_table(case, t)))


# ---------------------------------------------------------------------------------------------------------------- the solvers' own H / W
@pytest.mark.parametrize("name", ["ddim_cfg++", "dpm++_2m_cfgpp", "euler_cfg++"])
def test_sdxl_jobs_take_target_size_as_height_and_width(name):
    """target_size = (height, width), the order of the time_ids: a 64 x 192 job starts from an (8, 24) latent, not from its transpose
    (every other SDXL test asks for a square image)"""
    import types
    from cfgpp_amd.latent_sdxl import get_solver
    from cfgpp_amd.unet_config import TINY_XL as cfg
    from mock_engine import MockEngine
    seen = []

    def unet(z, t, ehs, te, ti):
        seen.append((tuple(z.shape), ti[0].tolist()))
        return (z.float() * 0.1).half()
    hw = (8, 24)
    s = get_solver(name, solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", unet_config=cfg, max_batch=1, latent_hw=hw,
                   engine=MockEngine(unet, hw), scalar_semantics="cuda")
    p = ["bad", "a cat"]
    out = s.sample(prompt1=p, prompt2=p, cfg_guidance=0.6, target_size=(64, 192), original_size=(64, 192), seeds=[1], return_latents=True)
    out = out[0] if isinstance(out, (tuple, list)) else out
    assert tuple(out.shape) == (1, 4) + hw
    assert seen and all(shape == (2, 4) + hw and ti == [64.0, 192.0, 0.0, 0.0, 64.0, 192.0] for shape, ti in seen)
