"""CPU: the loud weights of tests/loud_cases.py are loud (condition A: every fault of every kind on every key, and every input fault,
moves the fp32 oracle by at least 4 T), still reachable by an fp16 engine (condition B: rounding the weights to fp16 moves it by
less than T / 4), the silent keys are exactly the VAE attentions' to_k.bias for the stated reason, the fault tables reach every
key, ``explain`` names a planted fault, and profiles/loud_weights/quiet_keys.json - the gap the SYNTH weights leave - is
reproduced.  T is the tolerance of the existing GPU test of each engine (loud_cases.T_UNET / T_VAE), nothing measured here."""
import json
import os

import pytest
import torch

import loud_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITEMS = [(n, k) for n in L.ENGINES for k in L.KINDS if not (k == "halves" and n.startswith("vae"))]


def test_tolerances_are_the_existing_tests():
    import test_gpu_controlnet
    import test_gpu_unet
    assert L.T_UNET == test_gpu_unet.EPS_REL == test_gpu_controlnet.EPS_REL == 2.5e-3
    with open(os.path.join(ROOT, "tests", "test_gpu_vae.py")) as f:
        src = f.read()
    assert L.T_VAE == 1e-2 and "rel < 1e-2" in src and "rel_m < 1e-2 and rel_z < 1e-2 and rel_mean < 1e-2" in src


@pytest.mark.parametrize("name", L.ENGINES)
def test_loud_weights_are_the_synth_weights_rescaled(name):
    e, s = L.engine(name), L.engine(name, "synth")
    assert list(e.sd) == list(s.sd) and all(e.sd[k].shape == s.sd[k].shape and e.sd[k].dtype == torch.float32 for k in e.sd)
    again = type(e)(name, "loud")
    assert all(torch.equal(again.sd[k], e.sd[k]) for k in e.sd) and all(torch.equal(again.inputs[k], e.inputs[k]) for k in e.inputs
                                                                        if torch.is_tensor(e.inputs[k]))
    if not name.startswith("vae"):      # oracle and engine read the same bits
        assert all(torch.equal(v.half().float(), v) for v in e.sd.values())
    for k, v in e.sd.items():           # a rescaling: every element is the synth element's affine image, no tensor is redrawn
        u = s.sd[k].float()
        if L.is_norm(k) and k.endswith(".weight"):
            u, v = u - 1, v - 1
        ratio = (v.double() @ u.double()) / (u.double() @ u.double()) if v.dim() == 1 else (v.double() * u.double()).sum() / (u.double() ** 2).sum()
        assert torch.allclose(v.double(), u.double() * ratio, rtol=0, atol=2e-3 * float(v.abs().max())), k
    # all rows of every input differ: a row read from the wrong place shows
    for k, x in e.inputs.items():
        if torch.is_tensor(x) and x.dim() > 1 and x.shape[0] > 1 and k != "ti":
            assert all(not torch.equal(x[i], x[j]) for i in range(x.shape[0]) for j in range(i))


@pytest.mark.parametrize("name", L.ENGINES)
def test_fault_tables_reach_every_key(name):
    e = L.engine(name)
    sd = e.sd
    drops = e.faults("drop")
    assert [f.name for f in drops] == e.keys
    for f in drops[:3] + drops[-3:]:
        new, _ = f.apply(sd, e.inputs)
        changed = [k for k in sd if not torch.equal(new[k], sd[k])]
        assert changed == [f.name] and torch.equal(new[f.name], L.drop_value(f.name, sd[f.name]))
    square = [k for k, v in sd.items() if k.endswith(".weight") and v.dim() in (2, 4) and v.shape[0] == v.shape[1]]
    conv3 = [k for k, v in sd.items() if v.dim() == 4 and v.shape[-1] == 3]
    geglu = [k for k in sd if k.endswith("ff.net.0.proj.weight")]
    assert [f.name for f in e.faults("transpose")] == square and len(square) > 10
    assert len(e.faults("taps")) == 2 * len(conv3) and len(conv3) > 10
    assert [f.name for f in e.faults("halves")] == geglu and (bool(geglu) != name.startswith("vae"))
    swaps = [f.name for f in e.faults("swap")]
    assert len(set(swaps)) == len(swaps)
    kinds = ((".norm1.", ".norm2."), (".to_k.", ".to_v."), (".conv1.", ".conv2."), (".to_q.", ".to_out.0."), (".resnets.0.", ".resnets.1."))
    for a, b in kinds:
        assert any(a in s.split(" <-> ")[0] and b in s.split(" <-> ")[1] for s in swaps), (a, b)
    if not name.startswith("vae"):
        assert any(".norm3." in s for s in swaps)
    f = e.faults("swap")[0]
    a, b = f.name.split(" <-> ")
    new, _ = f.apply(sd, e.inputs)
    assert torch.equal(new[a], sd[b]) and torch.equal(new[b], sd[a]) and sd[a].shape == sd[b].shape and not torch.equal(sd[a], sd[b])
    # a fault that changes nothing could not be loud; the sweep below would say so, this names the table instead
    for kind in ("transpose", "taps", "halves"):
        for f in e.faults(kind)[:2]:
            new, _ = f.apply(sd, e.inputs)
            assert any(not torch.equal(new[k], sd[k]) for k in sd), f.name
    assert len(e.input_faults()) >= 1


@pytest.mark.parametrize("name,kind", ITEMS)
def test_condition_a_every_fault_is_loud(name, kind):
    e = L.engine(name)
    need = 4 * e.T
    res = L.sweep(name, kind, stop_at=need)
    assert res
    silent = [n for n, v in res if v < L.SILENT_BELOW]
    assert silent == (list(L.SILENT.get(name, ())) if kind == "drop" else []), silent
    quiet = sorted((v, n) for n, v in res if v < need and n not in silent)
    assert not quiet, f"{name} {kind}: {len(quiet)} of {len(res)} faults below 4 T = {need:g}: {quiet[:10]}"


@pytest.mark.parametrize("name", L.ENGINES)
def test_condition_b_fp16_weights_stay_inside_a_quarter_of_t(name):
    e = L.engine(name)
    for t in e.ts:
        r = e.rounding_effect(t)
        assert r < e.T / 4, (name, t, r)
        for o in e.base(t):           # and the loud nets stay far inside the fp16 range at their outputs
            assert torch.isfinite(o).all() and float(o.abs().max()) < 100.0


def test_silent_keys_are_the_vae_key_biases_and_for_the_stated_reason():
    assert set(L.SILENT) == {"vae_dec", "vae_enc"} and all(len(v) <= 1 for v in L.SILENT.values())
    assert all(k.endswith(".attentions.0.to_k.bias") for v in L.SILENT.values() for k in v)
    for name, keys in L.SILENT.items():
        e = L.engine(name)
        for k in keys:
            assert k in e.sd
            assert e.silent_reason(k, None) < L.SILENT_BELOW                 # a constant added to all of it: nothing changes
            drop = next(f for f in e.faults("drop") if f.name == k)
            assert e.effect(drop, None) < L.SILENT_BELOW
            # the bias is not silent because it is absent or tiny: the same values on to_v are loud
            v = k.replace(".to_k.", ".to_v.")
            moved = L.Fault("swap", "k <-> v", lambda sd, inputs, k=k, v=v: (dict(sd, **{k: sd[v], v: sd[k]}), inputs))
            assert e.effect(moved, None) >= 4 * e.T


def test_explain_names_a_planted_fault():
    e = L.engine("tiny_sd")
    t = 500.0
    faults = e.faults("drop")[::25] + e.input_faults()
    table = [(f"{f.kind}: {f.name}", L.flat(e.change(f, t))) for f in faults]
    g = torch.Generator().manual_seed(0)
    for i in (3, len(table) - 1):
        label, d = table[i]
        noise = torch.randn(d.shape, generator=g, dtype=torch.float64)
        noise *= 0.3 * d.norm() / noise.norm()
        top = L.explain(d + noise, table)
        assert len(top) == 3 and top[0][0] == label and top[0][1] > 0.9 and 0.9 < top[0][2] < 1.2, top
        assert abs(top[1][1]) < top[0][1]
        undone = L.explain([-(d + noise)], table)
        assert undone[0][0] == label and undone[0][1] < -0.9
    # pure noise accuses nobody: no cosine stands out
    assert all(abs(c) < 0.2 for _, c, _ in L.explain(torch.randn(table[0][1].shape, generator=g, dtype=torch.float64), table))


@pytest.mark.parametrize("name,kind", ITEMS)
def test_quiet_keys_of_the_synth_weights_as_recorded(name, kind):
    """documents the gap (it does NOT ask the synth weights to be loud): the recorded counts are reproduced"""
    with open(os.path.join(ROOT, "profiles", "loud_weights", "quiet_keys.json")) as f:
        rec = json.load(f)
    assert set(rec["engines"]) == set(L.ENGINES)
    assert rec["engines"][name]["keys"] == len(L.engine(name, "synth").keys)
    got = L.quiet_count(name, kind)
    assert got == rec["engines"][name][kind], (got, rec["engines"][name][kind])
    if kind == "drop":
        assert got["below_4T"] > 0          # there was a gap


def test_explain_refuses_another_layout():
    e = L.engine("controlnet")
    f = e.input_faults()[0]
    table = [(f.name, L.flat(e.change(f, 500.0)))]
    with pytest.raises(ValueError, match="another layout"):
        L.explain([e.base(500.0)[-1]], table)          # the controlled eps alone, not residuals + eps
