"""Long and weighted prompts (cfgpp_amd/prompt.py), no GPU: the parser's pins, the chunk borders, the over-limit error, the
padding of the shorter side with empty-prompt chunks, bit identity of a one-chunk unweighted prompt with the default path for
every tokenizer and a real (one-layer) CLIP tower, the weights' token rows, SDXL's pooled output and the solver plumbing on the
mock engine of tests/test_solver_cpu.py."""
import types

import pytest
import torch

import cfgpp_amd.latent_diffusion as sd
import cfgpp_amd.latent_sdxl as xl
from cfgpp_amd import prompt as P
from cfgpp_amd.conditioning import ClipBpeTokenizer, ClipTextTower, HashTokenizer, SyntheticTextEncoder
from mock_engine import MockEngine, StubVAE
from test_capi_and_config import _toy_clip_vocab

PINS = [
    ("normal text", [["normal text", 1.0]]),
    ("an (important) word", [["an ", 1.0], ["important", 1.1], [" word", 1.0]]),
    ("(unbalanced", [["unbalanced", 1.1]]),
    ("\\(literal\\]", [["(literal]", 1.0]]),
    ("(unnecessary)(parens)", [["unnecessaryparens", 1.1]]),
    ("a (((house:1.3)) [on] a (hill:0.5), sun, (((sky))).",
     [["a ", 1.0], ["house", 1.5730000000000004], [" ", 1.1], ["on", 1.0], [" a ", 1.1], ["hill", 0.55], [", sun, ", 1.1],
      ["sky", 1.4641000000000006], [".", 1.1]]),
]


@pytest.mark.parametrize("text,want", PINS, ids=[p[0] for p in PINS])
def test_parse_pins(text, want):
    got = P.parse_prompt_attention(text)
    assert [f for f, _ in got] == [f for f, _ in want]
    assert all(abs(g[1] - w[1]) <= 1e-12 for g, w in zip(got, want))


def test_parse_break_and_empty():
    assert P.parse_prompt_attention("") == [["", 1.0]]
    assert P.parse_prompt_attention("a cat BREAK (a dog:1.2)") == [["a cat", 1.0], ["BREAK", None], ["a dog", 1.2]]
    assert P.parse_prompt_attention("break") == [["break", 1.0]]          # the upper-case word only


def test_a_negative_weight_is_a_weight_not_a_break():
    assert P.parse_prompt_attention("a (b:-0.5) c") == [["a ", 1.0], ["b", -0.5], [" c", 1.0]]
    assert P.parse_prompt_attention("((b:-0.5))")[0][1] == pytest.approx(-0.55)          # nesting still multiplies
    tok = HashTokenizer()
    ids, w = P.chunk_prompt(tok, "a (b:-0.5) c", 4)
    assert ids.shape == (1, 77) and ids[0, 1:4].tolist() == tok.encode("a b c")             # nothing dropped, no chunk closed
    assert w[0, :5].tolist() == [1.0, 1.0, -0.5, 1.0, 1.0]


def words(n, start=0):
    return " ".join(f"w{start + i}" for i in range(n))


def bpe():
    vocab, merges = _toy_clip_vocab()
    return ClipBpeTokenizer(vocab, [" ".join(m) for m in merges])


@pytest.mark.parametrize("n,chunks,last", [(0, 1, 0), (75, 1, 75), (76, 2, 1), (150, 2, 75), (151, 3, 1)])
def test_chunk_borders(n, chunks, last):
    tok = HashTokenizer()
    text = words(n)                                    # (every "w<i>" is one id of the HashTokenizer)
    assert len(tok.encode(text)) == n
    ids, w = P.chunk_prompt(tok, text, 4)
    assert ids.shape == w.shape == (chunks, 77) and bool((w == 1).all())
    flat = []
    for r in range(chunks):
        k = 75 if r < chunks - 1 else last
        assert int(ids[r, 0]) == tok.BOS and int(ids[r, 1 + k]) == tok.EOS and bool((ids[r, 2 + k:] == tok.pad_id).all())
        flat += ids[r, 1: 1 + k].tolist()
    assert flat == tok.encode(text)                    # hard cut: nothing dropped, nothing moved


def test_break_closes_a_chunk_and_weights_follow_their_ids():
    tok = HashTokenizer(pad_id=0)
    ids, w = P.chunk_prompt(tok, "a (b c:1.5) BREAK [d] e", 4)
    assert ids.shape == (2, 77)
    assert ids[0, :5].tolist() == [tok.BOS] + tok.encode("a b c") + [tok.EOS] and bool((ids[0, 5:] == 0).all())
    assert w[0, :6].tolist() == [1.0, 1.0, 1.5, 1.5, 1.0, 1.0]
    assert ids[1, :4].tolist() == [tok.BOS] + tok.encode("d e") + [tok.EOS]
    assert torch.allclose(w[1, :4], torch.tensor([1.0, 1 / 1.1, 1.0, 1.0]))


def test_over_limit_is_an_error_that_names_the_counts():
    tok = HashTokenizer()
    with pytest.raises(ValueError, match=r"prompt of 151 tokens needs 3 chunks.*max_prompt_chunks=2 \(150 tokens"):
        P.chunk_prompt(tok, words(151), 2)
    P.chunk_prompt(tok, words(150), 2)
    with pytest.raises(ValueError, match="max_prompt_chunks=2"):
        P.chunk_prompt(tok, "a BREAK b BREAK c", 2)


def test_hash_tokenizer_encode_is_its_call_without_the_cut():
    tok = HashTokenizer()
    for text in ("a photo of a cat, 4k!", words(90), ""):
        e = tok.encode(text)
        row = tok([text])[0]
        k = min(len(e), 75)
        assert row[1: 1 + k].tolist() == e[:k] and int(row[1 + k]) == tok.EOS


@pytest.mark.parametrize("make", [HashTokenizer, lambda: HashTokenizer(pad_id=0), bpe], ids=["hash", "hash-pad0", "bpe"])
def test_one_chunk_ids_are_todays(make):
    tok = make()
    for text in ("a photo of an astronaut riding a horse", "", "hello, world! it's 2 good", words(75), words(20)):
        if len(tok.encode(text)) > 75:                 # (byte-level BPE spends several ids on a "w<i>")
            continue
        ids, w = P.chunk_prompt(tok, text.replace("(", "\\(").replace(")", "\\)"), 4)
        assert torch.equal(ids, tok([text])) and bool((w == 1).all())


def test_one_chunk_identity_with_a_clip_tower():
    """ClipTextTower.clip_l(layers=1) on the miniature vocabulary: an unweighted prompt of <= 75 ids gives today's tensors, bit for bit"""
    tower = ClipTextTower.clip_l(layers=1, tokenizer=bpe())
    prompts = ["a photo of a cat", "", "two words"]
    h0, p0 = tower(prompts)
    h1, p1 = P.encode_prompts(tower, prompts, 4)
    assert h1.shape == (3, 77, 768) and h1.dtype == torch.float16 and torch.equal(h0.view(torch.int16), h1.view(torch.int16))
    assert p0 is None and p1 is None
    he, _ = tower.encode_ids(tower.tok(prompts))
    assert torch.equal(he.view(torch.int16), h0.view(torch.int16))


def test_weights_land_on_their_token_rows_and_chunks_concatenate():
    enc = SyntheticTextEncoder(64, 32)
    tok = enc.tok
    text = "a (b:1.5) " + words(80) + " [z]"
    ids, w = P.chunk_prompt(tok, text, 4)
    assert ids.shape[0] == 2
    h, pooled = P.encode_prompts(enc, [text, "short"], 4)
    assert h.shape == (2, 154, 64) and pooled.shape == (2, 32)
    raw, praw = enc.encode_ids(ids)
    want = (raw.reshape(154, 64).float() * w.reshape(154, 1)).half()
    assert torch.equal(h[0], want)
    assert float(w[0, 2]) == 1.5 and torch.equal(h[0, 2], (raw[0, 2].float() * 1.5).half()) and torch.equal(h[0, 1], raw[0, 1])
    assert abs(float(w[1, 8]) - 1 / 1.1) < 1e-6          # 83 ids: "z" is id 7 of chunk 1
    assert torch.equal(pooled[0], praw[0])               # chunk 0, unweighted
    # the short prompt: its chunk, then a chunk of the empty prompt
    e_ids, _ = P.chunk_prompt(tok, "", 4)
    s_ids, _ = P.chunk_prompt(tok, "short", 4)
    he, _ = enc.encode_ids(torch.cat([s_ids, e_ids]))
    assert torch.equal(h[1], he.reshape(154, 64))


# ---- solver plumbing ----------------------------------------------------------------------------------------------------------
def cfgn(n):
    return types.SimpleNamespace(num_sampling=n)


def seen_unet(log):
    def fn(z, t, ehs, te, ti):
        log.append((tuple(ehs.shape), None if te is None else tuple(te.shape)))
        return torch.zeros_like(z).half()
    return fn


def test_sd_solver_pads_uc_to_the_prompts_chunks():
    log = []
    eng = MockEngine(seen_unet(log))
    s = sd.get_solver("ddim_cfg++", solver_config=cfgn(2), device="cpu", engine=eng, text_encoder=SyntheticTextEncoder(768),
                      latent_hw=(8, 8), vae=StubVAE(0.18215), max_prompt_chunks=3)
    long = "a (castle:1.3) " + words(160)
    uc, c = s.get_text_embed("", [long, "short"])
    assert uc.shape == (1, 231, 768) and c.shape == (2, 231, 768)
    enc = s.text_encoder
    e_ids, _ = P.chunk_prompt(enc.tok, "", 4)
    assert torch.equal(uc[0], enc.encode_ids(e_ids.expand(3, -1))[0].reshape(231, 768))      # three empty-prompt chunks
    s.sample(prompt=["", long], cfg_guidance=0.6, return_latents=True)
    assert log and all(shape == (2, 231, 768) for shape, _ in log)
    log.clear()
    s.sample(prompt=["", "one chunk"], cfg_guidance=0.6, return_latents=True)
    assert log and all(shape == (2, 77, 768) for shape, _ in log)
    with pytest.raises(ValueError, match="max_prompt_chunks=3"):
        s.get_text_embed("", words(226))
    pe = (torch.zeros(1, 154, 768), torch.zeros(1, 154, 768))
    log.clear()
    s.sample(prompt_embeds=pe, cfg_guidance=0.6, return_latents=True)
    assert log and all(shape == (2, 154, 768) for shape, _ in log)


def test_default_solver_is_untouched():
    """max_prompt_chunks = 1: no parsing - the encoder sees the prompt string, brackets and all"""
    seen = []

    class Enc:
        def __call__(self, prompts):
            seen.extend(prompts)
            return torch.zeros(len(prompts), 77, 768, dtype=torch.float16), None
    s = sd.get_solver("ddim_cfg++", solver_config=cfgn(2), device="cpu", engine=MockEngine(seen_unet([])), text_encoder=Enc(),
                      latent_hw=(8, 8), vae=StubVAE(0.18215))
    assert s.max_prompt_chunks == 1
    s.get_text_embed("", "(literal:1.3) BREAK")
    assert seen == ["", "(literal:1.3) BREAK"]
    with pytest.raises(ValueError, match="max_prompt_chunks=5"):
        sd.get_solver("ddim_cfg++", solver_config=cfgn(2), device="cpu", engine=MockEngine(seen_unet([])), max_prompt_chunks=5)
    with pytest.raises(ValueError, match="ip_adapter=... together with max_prompt_chunks=2"):
        sd.get_solver("ddim_cfg++", solver_config=cfgn(2), device="cpu", engine=MockEngine(seen_unet([])), max_prompt_chunks=2,
                      ip_adapter="synthetic")


def test_sdxl_chunks_both_towers_alike_and_pools_chunk_zero():
    log = []
    eng = MockEngine(seen_unet(log))
    e1, e2 = SyntheticTextEncoder(768, 1280, tag="clip_l"), SyntheticTextEncoder(1280, 1280, tag="clip_g")
    s = xl.get_solver("ddim_cfg++", solver_config=cfgn(2), device="cpu", engine=eng, text_encoder=(e1, e2), latent_hw=(8, 8),
                      vae=StubVAE(0.13025), max_prompt_chunks=2)
    long, short = "(x:1.2) " + words(100), "a cat"
    ne, pe, pool_null, pool = s.get_text_embed("", long, "", short)        # tower 1 needs two chunks, tower 2 one: both get two
    assert ne.shape == pe.shape == (1, 154, 2048) and pool.shape == pool_null.shape == (1, 1280)
    h2, p2 = P.encode_prompts(e2, [short], 2, n_chunks=2)
    assert torch.equal(pe[:, :, 768:], h2) and torch.equal(pool, p2)
    ids0, _ = P.chunk_prompt(e2.tok, short, 2)
    assert torch.equal(pool, e2.encode_ids(ids0)[1])                       # chunk 0 of tower 2, unweighted
    h1, _ = P.encode_prompts(e1, [long], 2)
    assert torch.equal(pe[:, :, :768], h1)
    s.sample(prompt1=["", long], prompt2=["", short], cfg_guidance=0.6, return_latents=True)
    assert log and all(shape == (2, 154, 2048) and te == (2, 1280) for shape, te in log)


def test_long_prompt_header_matches_its_prototype_table():
    """include/cfgpp_long_prompt.h: every declaration has a ctypes prototype in its own table (include/cfgpp.h stays at its size)"""
    import os
    import re
    from cfgpp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "cfgpp_long_prompt.h")).read()
    declared = set(re.findall(r"^int (cfgpp_[a-z0-9_]+)\(", hdr, re.M))
    assert declared == {"cfgpp_unet_set_max_tokens"} == set(_lib.LONG_PROMPT_PROTOTYPES)
    from cfgpp_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    for name, (res, args) in _lib.LONG_PROMPT_PROTOTYPES.items():      # exported, and bound with this table's types
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert not set(_lib.LONG_PROMPT_PROTOTYPES) & (set(_lib.PROTOTYPES) | set(_lib.DEBUG_PROTOTYPES) | set(_lib.IP_ADAPTER_PROTOTYPES))


def test_sdxl_null_prompt_2_alone_goes_through_tower_2_as_on_the_default_path():
    e1, e2 = SyntheticTextEncoder(768, 1280, tag="clip_l"), SyntheticTextEncoder(1280, 1280, tag="clip_g")
    s = xl.get_solver("ddim_cfg++", solver_config=cfgn(2), device="cpu", engine=MockEngine(seen_unet([])), text_encoder=(e1, e2),
                      latent_hw=(8, 8), vae=StubVAE(0.13025), max_prompt_chunks=2)
    ne, pe, pool_null, pool = s.get_text_embed("bad", "a cat", null_prompt_2="worse", prompt_2=None)
    assert ne.shape == (1, 77, 2048) and pe.shape == (1, 77, 768)
    h2, p2 = P.encode_prompts(e2, ["worse"], 2)
    assert torch.equal(ne[:, :, 768:], h2) and torch.equal(pool_null, p2)          # tower 2 encodes it, and pools the uncond side
    assert torch.equal(pool, P.encode_prompts(e1, ["a cat"], 2)[1])


def test_clip_skip_is_refused_not_dropped_on_the_long_path():
    enc = SyntheticTextEncoder(64, 32)
    with pytest.raises(NotImplementedError, match="clip_skip=1"):
        P.encode_prompts(enc, ["a cat"], 2, clip_skip=1)

    class NoKeyword(SyntheticTextEncoder):
        def encode_ids(self, ids):
            return super().encode_ids(ids)
    with pytest.raises(NotImplementedError, match="clip_skip=1.*NoKeyword"):
        P.encode_prompts(NoKeyword(64, 32), ["a cat"], 2, clip_skip=1)


def test_long_context_in_a_sharded_run_is_refused_for_prompt_embeds_too(monkeypatch):
    import torch.distributed as dist
    log = []
    s = sd.get_solver("ddim_cfg++", solver_config=cfgn(2), device="cpu", engine=MockEngine(seen_unet(log)), text_encoder=SyntheticTextEncoder(768),
                      latent_hw=(8, 8), vae=StubVAE(0.18215), max_prompt_chunks=2)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    pe = (torch.zeros(1, 154, 768), torch.zeros(1, 154, 768))
    with pytest.raises(ValueError, match=r"154 tokens \(2 prompt chunks\) in a sharded run"):
        s.sample(prompt_embeds=pe, cfg_guidance=0.6, return_latents=True)
    assert not log
    with pytest.raises(ValueError, match="in a sharded run"):
        s.get_text_embed("", "a " + words(80))
    s.sample(prompt_embeds=(torch.zeros(1, 77, 768), torch.zeros(1, 77, 768)), cfg_guidance=0.6, return_latents=True)      # one chunk: fine
    assert log


def test_a_type_error_inside_encode_ids_is_not_taken_for_a_missing_keyword():
    class Broken(SyntheticTextEncoder):
        def encode_ids(self, ids, clip_skip=None):
            raise TypeError("inside the tower")
    with pytest.raises(TypeError, match="inside the tower"):
        P.encode_prompts(Broken(64, 32), ["a cat"], 2, clip_skip=1)
