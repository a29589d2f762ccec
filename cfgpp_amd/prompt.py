"""Long and weighted prompts (opt-in: ``get_solver(..., max_prompt_chunks=K)`` with K = 2 .. 4).

With ``max_prompt_chunks=1`` (the default) nothing here runs: a prompt is cut at 75 ids and brackets are literal text, as in the
reference.  With K > 1 a prompt goes through three steps:

parse   ``parse_prompt_attention``: the emphasis syntax other Stable Diffusion front ends share - ``(x)`` multiplies the weight
        of x by 1.1, ``[x]`` divides it by 1.1, ``(x:w)`` multiplies it by w, nesting multiplies, ``\\( \\) \\[ \\]`` are literal
        brackets, an unclosed bracket applies to the end of the prompt, the upper-case word ``BREAK`` ends a chunk.
chunk   ``chunk_prompt``: every fragment is tokenised on its own (the tokenizer's ``encode``: no BOS / EOS) and every id carries
        its fragment's weight; the ids are cut HARD every 75 - there is no look-back to the last comma - and ``BREAK`` closes the
        current chunk; each chunk becomes ``[BOS] + ids + [EOS] + pad...`` of 77 ids in the tokenizer's own pad layout, with
        weight 1 on BOS / EOS / pad.  An empty prompt is one chunk.  More than K chunks is an error, never a silent cut.
encode  ``encode_prompts``: the chunks go through the text encoder's ``encode_ids`` as batch rows, the hidden states are
        concatenated along the token axis to ``[n, 77 * j, D]`` and every token row is multiplied by its weight in fp32, then
        rounded to fp16.  The mean of the weighted states is NOT restored to that of the unweighted ones (some front ends do):
        the seeded synthetic embeddings this project runs on have mean ~ 0, and a ratio of two such means is noise.  The pooled
        output is that of chunk 0, unweighted.  Prompts of one batch - and the unconditional and conditional side of a call -
        are padded with chunks of the empty prompt to the longest chunk count.

A prompt of at most 75 ids whose weights are all 1 gives, bit for bit, the tensors of the default path - with the encoders that
are a tokenizer plus a tower (``ClipTextTower``, the HIP tower of ``text.py``).  ``SyntheticTextEncoder`` is the exception: its
``__call__`` is seeded by the prompt's text, its ``encode_ids`` by the id row (a chunk has no text of its own), so the two paths
give different - equally distributed - tensors.  ``clip_skip`` reaches ``encode_ids`` as a keyword; an encoder that cannot honour
it refuses (NotImplementedError), it is never dropped.
"""
from __future__ import annotations

import inspect
import re
from typing import List, Optional, Sequence, Tuple

import torch

CHUNK_IDS = 75                  # ids per chunk; with BOS and EOS the 77 tokens of a CLIP context
CHUNK_TOKENS = 77
MAX_CHUNKS = 4                  # include/cfgpp_long_prompt.h: cfgpp_unet_set_max_tokens takes up to 308 = 4 x 77
BREAK = "BREAK"

_TOKEN = re.compile(r"\\[()\[\]\\]|\\|\(|\[|:\s*([+-]?(?:\d+\.?\d*|\.\d+))\s*\)|\)|\]|[^\\()\[\]:]+|:")
_BREAK = re.compile(r"\s*\bBREAK\b\s*")


def parse_prompt_attention(text: str) -> List[list]:
    """``text`` -> ``[[fragment, weight], ...]``; a chunk break is the pair ``["BREAK", None]`` - no weight at all, so that a
    negative weight, ``(word:-0.5)``, stays a weight"""
    out: List[list] = []
    round_open: List[int] = []          # index into `out` where each open bracket starts
    square_open: List[int] = []

    def scale(start, m):
        for frag in out[start:]:
            if frag[1] is not None:     # (a break carries no weight)
                frag[1] *= m

    for m in _TOKEN.finditer(text):
        tok, weight = m.group(0), m.group(1)
        if tok.startswith("\\") and len(tok) == 2:
            out.append([tok[1], 1.0])
        elif tok == "(":
            round_open.append(len(out))
        elif tok == "[":
            square_open.append(len(out))
        elif weight is not None and round_open:
            scale(round_open.pop(), float(weight))
        elif tok == ")" and round_open:
            scale(round_open.pop(), 1.1)
        elif tok == "]" and square_open:
            scale(square_open.pop(), 1 / 1.1)
        else:
            parts = _BREAK.split(tok)
            for i, part in enumerate(parts):
                if i > 0:
                    out.append([BREAK, None])
                out.append([part, 1.0])
    for start in round_open:            # unclosed brackets reach to the end of the prompt
        scale(start, 1.1)
    for start in square_open:
        scale(start, 1 / 1.1)
    merged: List[list] = []
    for frag, w in out:
        if merged and w is not None and merged[-1][1] == w:
            merged[-1][0] += frag
        elif frag != "" or w is None:
            merged.append([frag, w])
    # an empty fragment next to a break (or alone) says nothing
    if not merged:
        merged = [["", 1.0]]
    return merged


def tokenizer_of(encoder):
    tok = getattr(encoder, "tok", None)
    if tok is None or not hasattr(tok, "encode"):
        raise ValueError(f"max_prompt_chunks > 1: the text encoder {type(encoder).__name__} exposes no tokenizer with an `encode` method "
                         "(attribute `tok`)")
    return tok


def _chunk_row(tok, ids: Sequence[int], weights: Sequence[float]):
    row = torch.full((CHUNK_TOKENS,), int(tok.pad_id), dtype=torch.long)
    w = torch.ones((CHUNK_TOKENS,), dtype=torch.float32)
    full = [int(tok.BOS)] + [int(i) for i in ids] + [int(tok.EOS)]
    row[: len(full)] = torch.tensor(full)
    if len(ids):
        w[1: 1 + len(ids)] = torch.tensor(list(weights), dtype=torch.float32)
    return row, w


def chunk_prompt(tok, text: str, max_chunks: int = MAX_CHUNKS) -> Tuple[torch.Tensor, torch.Tensor]:
    """``text`` -> (ids [j, 77] long, weights [j, 77] fp32), 1 <= j <= ``max_chunks``.  Hard cut every 75 ids (no comma look-back);
    ``BREAK`` closes the current chunk; raises when the prompt needs more than ``max_chunks`` chunks."""
    chunks, cur_i, cur_w, total = [], [], [], 0

    def close():
        chunks.append((list(cur_i), list(cur_w)))
        cur_i.clear()
        cur_w.clear()

    for frag, w in parse_prompt_attention(text):
        if w is None:
            close()
            continue
        for i in tok.encode(frag):
            if len(cur_i) == CHUNK_IDS:
                close()
            cur_i.append(i)
            cur_w.append(w)
            total += 1
    if cur_i or not chunks:
        close()
    if len(chunks) > max_chunks:
        raise ValueError(f"prompt of {total} tokens needs {len(chunks)} chunks of {CHUNK_IDS}: the limit is max_prompt_chunks={max_chunks} "
                         f"({CHUNK_IDS * max_chunks} tokens; BREAK closes a chunk early) - nothing is cut silently")
    rows = [_chunk_row(tok, i, w) for i, w in chunks]
    return torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])


def chunks_needed(encoder, prompts: Sequence[str], max_chunks: int) -> int:
    """the chunk count of the longest of ``prompts`` under ``encoder``'s tokenizer"""
    tok = tokenizer_of(encoder)
    return max(int(chunk_prompt(tok, p, max_chunks)[0].shape[0]) for p in prompts)


def encode_prompts(encoder, prompts: Sequence[str], max_chunks: int, n_chunks: Optional[int] = None, clip_skip: Optional[int] = None):
    """-> (hidden [n, 77 * j, D] fp16, pooled of chunk 0 | None) with j = max(longest prompt's chunks, ``n_chunks``): shorter
    prompts are padded with chunks of the empty prompt"""
    tok = tokenizer_of(encoder)
    if not hasattr(encoder, "encode_ids"):
        raise ValueError(f"max_prompt_chunks > 1: the text encoder {type(encoder).__name__} has no `encode_ids(ids [n, 77])`")
    cut = [chunk_prompt(tok, p, max_chunks) for p in prompts]
    j = max([int(i.shape[0]) for i, _ in cut] + [int(n_chunks or 1)])
    if j > max_chunks:
        raise ValueError(f"{j} prompt chunks asked for, the limit is max_prompt_chunks={max_chunks}")
    empty_i, empty_w = _chunk_row(tok, [], [])
    ids = torch.stack([torch.cat([i, empty_i.expand(j - i.shape[0], -1)]) for i, _ in cut])             # [n, j, 77]
    wts = torch.stack([torch.cat([w, empty_w.expand(j - w.shape[0], -1)]) for _, w in cut])
    n = len(cut)
    rows = ids.reshape(n * j, CHUNK_TOKENS)
    step = max(1, int(getattr(encoder, "max_batch", 8)))
    extra = {}
    if clip_skip is not None:           # asked of the signature, not of the call: a TypeError from inside a tower stays what it is
        params = inspect.signature(encoder.encode_ids).parameters
        if "clip_skip" not in params and not any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values()):
            raise NotImplementedError(f"clip_skip={clip_skip}: text encoder {type(encoder).__name__} returns one hidden state only "
                                      "(its encode_ids takes no clip_skip keyword)")
        extra["clip_skip"] = int(clip_skip)
    hs, pooled = [], []
    for s in range(0, n * j, step):
        h, p = encoder.encode_ids(rows[s: s + step], **extra)
        hs.append(h)
        pooled.append(p)
    h = torch.cat(hs)
    h = h.reshape(n, j * CHUNK_TOKENS, h.shape[-1])
    h = (h.float() * wts.reshape(n, j * CHUNK_TOKENS, 1).to(h.device)).to(torch.float16)
    if pooled[0] is None:
        return h, None
    p = torch.cat(pooled)
    return h, p.reshape(n, j, p.shape[-1])[:, 0].contiguous()
