"""Host-side packing of caller-given tokens for the decode loop (include/vitcap_hip.h: vitcap_engine_generate_forced).

One array describes both uses: ``forced`` int64 (rows, max_length), column 0 ignored, -1 = the step chooses freely, a token id =
the sequence takes that token at that position if it is still unfinished there.

* a caption PREFIX (``prefix_ids``): the reference's step loops run from any ``cur_len`` (``_generate_no_beam_search(input_ids,
  cur_len, ...)``, modeling_utils.py:768-886) and score the generated tokens only -> ``score_forced = 0``;
* a whole CAPTION to score (``caption_ids``): every position up to and including the first [SEP] is forced and enters the
  score like a chosen token (modeling_utils.py:850-877 on given words) -> ``score_forced = 1``.  One position is special: a
  [SEP] in the LAST column of a caption that has not ended before it.  generate() writes it there whatever was chosen
  (modeling_utils.py:870-871) while its score holds the chosen token's log-prob, so the returned ids do not say what to force.
  That column is left free -- the loop takes its argmax, as greedy decoding did, and score(generate(x)) is generate's own score
  -- unless the caller knows the token (``last_tok``, e.g. the engine's out_last_tok of a sampled sequence).

No GPU is involved: plain torch on the host.
"""
import torch

from ._lib import VOCAB

BOS, EOS, PAD, FREE = 101, 102, 0, -1


def _as_rows(x, rows, what):
    t = torch.as_tensor(x)
    if t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError('%s must hold integer token ids, got %s' % (what, t.dtype))
    t = t.to(torch.int64).cpu()
    if t.dim() != 2 or t.shape[0] != rows:
        raise ValueError('%s must be (%d, n), got %s' % (what, rows, tuple(t.shape)))
    return t


def pack_forced(prefix_ids=None, caption_ids=None, rows=None, max_length=20, last_tok=None):
    """-> (forced int64 (rows, max_length) on the host, score_forced).

    prefix_ids  (rows, P): the tokens of positions 1..P, without [CLS]; shorter rows are padded with -1 behind their last token;
                P <= max_length - 1.
    caption_ids (rows, max_length): [CLS] first, [SEP]-terminated, 0-padded -- what generate() returns and tensorize_ab builds.
                Positions behind the first [SEP] are left free (the sequence has ended there; the kernels ignore them anyway).
                A row whose first [SEP] stands in the last column: that column is free, or last_tok[row] (rows,) when given.
    Refused: both or neither argument, wrong shapes, ids outside the vocabulary, a -1 followed by a token in a prefix row, a
    caption row that does not start with [CLS]."""
    if (prefix_ids is None) == (caption_ids is None):
        raise ValueError('pack_forced takes exactly one of prefix_ids and caption_ids')
    if rows is None or int(rows) < 1 or not 2 <= int(max_length) <= 40:
        raise ValueError('pack_forced needs rows >= 1 and max_length in 2..40 (got rows=%r, max_length=%r)' % (rows, max_length))
    rows, max_length = int(rows), int(max_length)
    forced = torch.full((rows, max_length), FREE, dtype=torch.int64)
    if prefix_ids is not None:
        p = _as_rows(prefix_ids, rows, 'prefix_ids')
        P = p.shape[1]
        if P > max_length - 1:
            raise ValueError('prefix_ids holds %d positions, max_length=%d leaves %d' % (P, max_length, max_length - 1))
        if bool(((p < FREE) | (p >= VOCAB)).any()):
            raise ValueError('prefix_ids holds ids outside -1 (padding) and the vocabulary 0..%d' % (VOCAB - 1))
        given = p != FREE
        if P > 1 and bool((~given[:, :-1] & given[:, 1:]).any()):
            raise ValueError('prefix_ids rows are -1-padded BEHIND their tokens: a token follows a -1')
        forced[:, 1:1 + P] = p
        return forced, 0
    c = _as_rows(caption_ids, rows, 'caption_ids')
    if c.shape[1] != max_length:
        raise ValueError('caption_ids must be (%d, %d), got %s' % (rows, max_length, tuple(c.shape)))
    if bool(((c < 0) | (c >= VOCAB)).any()):
        raise ValueError('caption_ids holds ids outside the vocabulary 0..%d' % (VOCAB - 1))
    if bool((c[:, 0] != BOS).any()):
        raise ValueError('caption_ids rows must start with [CLS] (%d)' % BOS)
    ended = (torch.cumsum((c[:, 1:] == EOS).long(), 1) - (c[:, 1:] == EOS).long()) > 0      # strictly behind the first [SEP]
    forced[:, 1:] = torch.where(ended, torch.full_like(c[:, 1:], FREE), c[:, 1:])
    by_rule = (c[:, -1] == EOS) & ~ended[:, -1]                    # the max-length rule's [SEP], not a choice
    fill = torch.full((rows,), FREE, dtype=torch.int64)
    if last_tok is not None:
        fill = torch.as_tensor(last_tok).to(torch.int64).cpu().reshape(-1)
        if fill.shape[0] != rows or bool(((fill < 0) | (fill >= VOCAB)).any()):
            raise ValueError('last_tok must hold %d token ids of the vocabulary' % rows)
    forced[:, -1] = torch.where(by_rule, fill, forced[:, -1])
    return forced, 1
