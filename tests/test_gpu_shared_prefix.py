"""-m gpu: the shared CFG prefix of the UNet forward (csrc/unet.hip).  A call with rows == 2 * z_rows on a net without
add_embedding runs the plan ops between conv_in and the first cross-attention on z_rows rows and fans the three live tensors out to
the upper rows.  The inputs of those ops are the same for rows r and r + z_rows, so the result may differ from the full-rows plan
only by the order of fp32 sums (the two-launch GroupNorm picks its block count from the row count, a K-split rule may pick
differently at M / 2): it must stay under the suite's forward tolerance against the fp32 oracle and be closer to the full-rows result
than that one is to the oracle."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS_REL = 2.5e-3        # tests/test_gpu_unet.py: per-forward eps rel-L2 against the fp32 CPU oracle


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


@pytest.fixture()
def switch():
    """the process-global switch, restored to its default (on) whatever the test did"""
    from cfgpp_amd import engine as E
    yield E.set_share_prefix
    if torch.cuda.is_available():
        E.set_share_prefix(True)


def _rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().float()


def _net(cfg, R, hw, seed=0):
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.weights import synth_state_dict
    sd = synth_state_dict(cfg, seed)
    net = HipUNet(cfg, max_rows=R, sample_hw=(hw, hw))
    net.load_state_dict(sd).finalize()
    return net, sd


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _half_rows_in_profile(net, z):
    """plan ops the profiler reports at another row count than the call's (its ' rows=N' suffix)"""
    detail = net.profile(z, 500.0, detail=True)["detail"]
    return [ln.split("\t")[2] for ln in detail.strip().split("\n") if " rows=" in ln.split("\t")[2]]


@pytest.mark.parametrize("R,hw", [(4, 16), (6, 24)])
def test_shared_prefix_vs_oracle_and_vs_full_rows(switch, R, hw):
    """tiny_sd at the shapes of test_unet_forward_vs_oracle, three ways: (a) shared, (b) full rows through the switch, (c) full rows
    by passing z already repeated to 2B rows - each against UNetRef; (b) == (c) bit for bit; rel-L2(a, b) <= rel-L2(b, oracle)"""
    need_gpu()
    from cfgpp_amd.unet_config import TINY_SD as cfg
    from oracle.unet_ref import UNetRef
    B = R // 2
    z = _rnd(B, 4, hw, hw, seed=50)
    ehs = _rnd(R, 77, cfg.cross_attention_dim, scale=0.5, seed=51)
    net, sd = _net(cfg, R, hw)
    net.set_context(ehs)
    ref_net = UNetRef(cfg, sd)
    zd, zz = z.cuda(), torch.cat([z, z]).cuda()
    for t in (981.0, 1.0):
        ref = ref_net(torch.cat([z, z]), t, ehs, None)["sample"]
        switch(True)
        assert net.shared_prefix_ops(R, B) > 0 and net.shared_prefix_ops(R, R) == 0
        a = net.forward(zd, t).clone()
        c = net.forward(zz, t).clone()                  # rows == z_rows: does not qualify, switch still on
        switch(False)
        assert net.shared_prefix_ops(R, B) == 0
        b = net.forward(zd, t).clone()
        ra, rb, rc, rab = _rel(a, ref), _rel(b, ref), _rel(c, ref), _rel(a, b)
        print(f"tiny_sd rows={R} hw={hw} t={t}: shared/oracle {ra:.3e}  switch-off/oracle {rb:.3e}  repeated-z/oracle {rc:.3e}  "
              f"shared/switch-off {rab:.3e}  shared bit-equal to full rows: {torch.equal(a, b)}")
        assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()
        assert ra < EPS_REL and rb < EPS_REL and rc < EPS_REL, (ra, rb, rc)
        assert torch.equal(b, c), "the two full-rows forms differ"
        assert rab <= rb, f"shared vs full rows {rab:.3e} > full rows vs oracle {rb:.3e}"


def test_mode_switching_on_one_engine_is_deterministic(switch):
    """shared, full rows, shared on ONE engine: the first and the third result are bit-equal (no stale pins, no stale upper rows of
    the prefix buffers, no missed fan-out), and each mode repeats itself"""
    need_gpu()
    from cfgpp_amd.unet_config import TINY_SD as cfg
    R, hw = 8, 32                                       # 32 x 32: the GroupNorms take their producers' statistics
    net, _ = _net(cfg, R, hw, seed=1)
    net.set_context(_rnd(R, 77, cfg.cross_attention_dim, scale=0.5, seed=7))
    z = _rnd(R // 2, 4, hw, hw, seed=8).cuda()
    switch(True)
    a1 = net.forward(z, 500.0).clone()
    a1b = net.forward(z, 500.0).clone()
    switch(False)
    b = net.forward(z, 500.0).clone()
    switch(True)
    a2 = net.forward(z, 500.0).clone()
    z2 = _rnd(R // 2, 4, hw, hw, seed=9).cuda()         # another latent in between: the upper rows now hold ITS prefix
    net.forward(z2, 321.0)
    a3 = net.forward(z, 500.0).clone()
    assert torch.isfinite(a1.float()).all()
    assert torch.equal(a1, a1b) and torch.equal(a1, a2) and torch.equal(a1, a3)
    assert _rel(a1, b) < EPS_REL
    # both halves of the batch went through the fan-out: with the same context on both halves they must be the same rows
    ctx = _rnd(R // 2, 77, cfg.cross_attention_dim, scale=0.5, seed=10)
    net.set_context(torch.cat([ctx, ctx]))
    e = net.forward(z, 500.0)
    assert torch.equal(e[: R // 2], e[R // 2:])


def test_calls_and_configs_that_do_not_qualify_are_unchanged(switch):
    """tiny_xl (per-row time embedding, no attention at level 0) and tiny_sd with z_rows == rows: bit-equal with the switch on and
    off, and neither the getter nor the profile shows an op at half rows"""
    need_gpu()
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    R, hw = 4, 16
    for cfg, zrows in ((TINY_XL, R // 2), (TINY_SD, R)):
        net, _ = _net(cfg, R, hw)
        te = ti = None
        if cfg.addition_embed:
            te = _rnd(R, cfg.addition_pooled_dim, scale=0.5, seed=52)
            ti = torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]] * R)
        net.set_context(_rnd(R, 77, cfg.cross_attention_dim, scale=0.5, seed=51), te, ti)
        z = _rnd(zrows, 4, hw, hw, seed=50).cuda()
        outs = []
        for on in (True, False, True):
            switch(on)
            assert net.shared_prefix_ops(R, zrows) == 0, (cfg.name, on)
            outs.append(net.forward(z, 700.0).clone())
            assert _half_rows_in_profile(net, z) == [], (cfg.name, on)
        assert torch.isfinite(outs[0].float()).all()
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), cfg.name
    # the qualifying call on the same kind of net does show them (the check above is not vacuous)
    switch(True)
    net, _ = _net(TINY_SD, R, hw)
    net.set_context(_rnd(R, 77, TINY_SD.cross_attention_dim, scale=0.5, seed=51))
    z = _rnd(R // 2, 4, hw, hw, seed=50).cuda()
    net.forward(z, 700.0)
    half = _half_rows_in_profile(net, z)
    assert len(half) == net.shared_prefix_ops(R, R // 2) + 1, half      # the prefix ops and the fan-out
    full = net.flops(R)
    switch(False)
    net.forward(z, 700.0)
    assert net.flops(R) > full                          # the shared prefix was counted once


def test_graph_replay_with_shared_prefix_is_bit_identical(monkeypatch, switch):
    """cfgpp_sample_graph_ddim on tiny_sd with the mode on: the captured step runs the same plan as the eager loop"""
    need_gpu()
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD as cfg
    switch(True)
    s = get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=7), device="cuda", unet_config=cfg, max_batch=2)
    uc, c = s.get_text_embed("bad", ["a cat", "a dog"])

    def run():
        return [t.clone() for t in s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), seeds=[5, 6], return_latents=True)]
    monkeypatch.setenv("CFGPP_GRAPH", "0")
    eager = run()
    monkeypatch.setenv("CFGPP_GRAPH", "1")
    graph = run()
    again = run()
    same = lambda a, b: all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))      # noqa: E731
    assert torch.isfinite(eager[0]).all()
    assert same(eager, graph) and same(eager, again)
    # the switch flipped between two graph calls: the cached graph of the other mode must not be replayed
    switch(False)
    off_graph = run()
    monkeypatch.setenv("CFGPP_GRAPH", "0")
    off_eager = run()
    assert same(off_eager, off_graph)
