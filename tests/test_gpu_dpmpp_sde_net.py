"""-m gpu: DPM++ SDE sampling on the HIP engine - 3-step chains (first step, middle step, last step with x' = D: 5 UNet calls) of both
families (tiny SD, tiny SDXL; 16 x 16 latents, 2 chains) against the same solver on a mock engine (tests/dpmpp_sde_mock.py) whose
UNet is the oracle and whose stage is the model of tests/dpmpp_sde_ref.py fed the model's Philox noise: the same seeds, therefore the
same noise.  Batched chains against independent runs, eta = 1 against eta = 0, and a plain `ddim_cfg++` job on the same engine before
and after a DPM++ SDE job.

Chain tolerances (the convention of tests/test_gpu_sde_net.py): the final denoised by rel-L2 against the oracle loop, under the
project's chain bar of 7.5e-3 (tests/test_gpu_pano_net.py) and under twice the value measured on the MI355X (CHAIN_MEASURED below;
profiles/dpmpp_sde/README.md).  Measured: tiny SD `dpm++_sde_cfg++` at 0.6 4.311e-4, tiny SDXL `dpm++_sde` at 7.5 3.345e-3, tiny SD
`dpm++_sde_cfg++` at eta = 0 3.469e-4, tiny SD v-prediction `dpm++_sde_cfg++` 7.306e-4; eta = 1 against eta = 0 moves the result by
0.48 .. 1.25."""
import types

import pytest
import torch

from dpmpp_sde_mock import DPMppSDEMockEngine

pytestmark = pytest.mark.gpu

CHAIN_BAR = 7.5e-3          # the project's chain bar (tests/test_gpu_pano_net.py)
H = torch.float16
N = 3
# (model, solver, options, cfg_guidance)
CASES = {
    "sd_cfgpp": ("sd15", "dpm++_sde_cfg++", {}, 0.6),
    "xl_cfg": ("sdxl", "dpm++_sde", {}, 7.5),
    "sd_cfgpp_eta0": ("sd15", "dpm++_sde_cfg++", dict(eta=0.0), 0.6),
    "sd_cfgpp_vpred": ("sd15", "dpm++_sde_cfg++", dict(prediction_type="v_prediction"), 0.6),
}
# measured rel-L2 of the 3-step chains below against the oracle loop -> asserted at twice the value (and under CHAIN_BAR)
CHAIN_MEASURED = {"sd_cfgpp": 4.311e-4, "xl_cfg": 3.345e-3, "sd_cfgpp_eta0": 3.469e-4, "sd_cfgpp_vpred": 7.306e-4}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def _cfg(model):
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    return TINY_SD if model == "sd15" else TINY_XL


def _sde(model, name, **kw):
    from cfgpp_amd.dpmpp_sde import get_dpmpp_sde_solver
    return get_dpmpp_sde_solver(name, model=model, solver_config=types.SimpleNamespace(num_sampling=N), unet_config=_cfg(model),
                                max_batch=2, latent_hw=(16, 16), scalar_semantics="cuda", **kw)


def _embeds(s, model):
    if model == "sd15":
        return s.get_text_embed("bad", ["a cat", "a dog"])
    return s.get_text_embed("bad", ["a cat", "a dog"], "bad", ["a cat", "a dog"])


def _sample(s, model, pe, seeds, lam, **kw):
    if model == "sd15":
        return s.sample(cfg_guidance=lam, prompt_embeds=pe, seeds=seeds, return_latents=True, **kw)
    return s.sample(cfg_guidance=lam, prompt_embeds=pe, target_size=(128, 128), original_size=(128, 128), seeds=seeds, return_latents=True, **kw)


class OracleMock(DPMppSDEMockEngine):
    """the mock engine whose UNet is the oracle"""

    def __init__(self, cfg, sd):
        from oracle.unet_ref import UNetRef
        self.net = UNetRef(cfg, sd)
        super().__init__(self._unet, (16, 16))

    def _unet(self, z, t, ehs, te, ti):
        ack = None if te is None else {"text_embeds": te.float(), "time_ids": ti.float()}
        return self.net(z.float(), t, ehs.float(), ack)["sample"].half()


@pytest.mark.parametrize("case", list(CASES))
def test_chain_vs_oracle_loop(case):
    need_gpu()
    from cfgpp_amd.weights import synth_state_dict
    model, name, opts, lam = CASES[case]
    cfg = _cfg(model)
    hip = _sde(model, name, device="cuda", **opts)
    eng = OracleMock(cfg, synth_state_dict(cfg, 0))
    ref = _sde(model, name, device="cpu", text_encoder=hip.text_encoder, engine=eng, **opts)
    pe = _embeds(hip, model)
    seeds = [11, 12]
    a_den, a_x = (t.clone() for t in _sample(hip, model, pe, seeds, lam))
    b_den, b_x = _sample(ref, model, tuple(x.cpu() for x in pe), seeds, lam)
    assert [n for n, _ in eng.scalls] == ["sde_input"] + ["step_sde_stage"] * (2 * N - 1) and len(eng.calls) == 2 * N - 1
    rel = rel_l2(a_den, b_den)
    # eta = 1 against eta = 0: the noise reaches the result
    other_eta = 1.0 if opts.get("eta") == 0.0 else 0.0
    other = _sample(_sde(model, name, device="cuda", engine=hip.engine, text_encoder=hip.text_encoder, **dict(opts, eta=other_eta)),
                    model, pe, seeds, lam)[0].clone()
    print(f"{case}: DPM++ SDE chain rel-L2 {rel:.3e}; eta {opts.get('eta', 1.0)} vs {other_eta} {rel_l2(a_den, other):.3e}")
    assert torch.isfinite(a_den).all() and torch.equal(a_den, a_x) and a_den.dtype == torch.float32 and float(a_den.std()) > 0
    assert rel < CHAIN_BAR, rel
    tol = 2 * CHAIN_MEASURED[case]
    assert rel < tol, rel
    assert rel_l2(a_den, other) > 10 * tol
    hip._ctx_key = None                                              # the other solver set the shared engine's context
    # batched chains equal independent runs, bit for bit
    for b in range(2):
        pe_b = tuple(x[b:b + 1] if x.shape[0] == 2 else x for x in pe)
        d1, _ = _sample(hip, model, pe_b, seeds[b:b + 1], lam)
        assert torch.equal(d1[0], a_den[b]), f"chain {b} alone differs from chain {b} of the batch"
    # the same seeds again: the same bits; other seeds: another result
    assert torch.equal(_sample(hip, model, pe, seeds, lam)[0], a_den)
    assert not torch.equal(_sample(hip, model, pe, [11, 13], lam)[0][1], a_den[1])


def test_plain_engine_gives_the_same_bits_around_a_dpmpp_sde_job():
    need_gpu()
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    mk = lambda: get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=5), device="cuda", unet_config=TINY_SD,  # noqa: E731
                            max_batch=2, latent_hw=(16, 16), scalar_semantics="cuda")
    s = mk()
    pe = s.get_text_embed("bad", ["a cat", "a dog"])
    run = lambda sv: [t.clone() for t in sv.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=[5, 6], return_latents=True)]  # noqa: E731
    before = run(s)
    sde = _sde("sd15", "dpm++_sde_cfg++", device="cuda", engine=s.engine, text_encoder=s.text_encoder)
    den, x = sde.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=[5, 6], return_latents=True)
    assert torch.isfinite(den).all()
    s._ctx_key = None                                                # the job set the engine's context: the next job sets its own
    after = run(s)
    fresh = run(mk())
    for a, b, w in zip(before, after, fresh):
        assert torch.equal(a, b) and torch.equal(a, w)
