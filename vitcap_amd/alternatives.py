"""Host helpers for the token alternatives of ImageCaptioning.alternatives() / caption_with_alternatives(): what the [MASK] probe saw
in the vocabulary at every position of a caption.  Per position the k best vocabulary entries (`ids`, best first, ties to the lower
id) with their log-probs, the rank of the scored word (0 = it is the model's first choice) and the entropy of the distribution in
nats.  Column 0 and the positions behind a caption's end hold ids = rank = -1 and logprobs = entropy = 0.  Works on torch tensors and
numpy arrays alike."""
import collections
import math

K_MAX = 16      # alternatives per position the kernel selects at most

Alternatives = collections.namedtuple('Alternatives', ['ids', 'logprobs', 'rank', 'entropy'])


def check_k(k):
    """k as the engine takes it -> int; anything else is refused by name."""
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= K_MAX:
        raise ValueError('alternatives: k must be 1..%d (got %r)' % (K_MAX, k))
    return int(k)


def _rows(a):
    return a.tolist() if hasattr(a, 'tolist') else list(a)


def to_words(tokenizer, alts, row):
    """Caption `row` of `alts` with words instead of ids: one list per position, [] at the dead positions, else k
    (word, log-prob) pairs, best first."""
    vocab = tokenizer.ids_to_tokens
    out = []
    for ids, lps in zip(_rows(alts.ids[row]), _rows(alts.logprobs[row])):
        out.append([(vocab[int(i)], float(p)) for i, p in zip(ids, lps) if int(i) >= 0])
    return out


def summary(token_logprobs, rank, ids, entropy=None):
    """Teacher-forced evaluation of a checkpoint on given captions, over the live positions (ids[..., 0] >= 0, where rank >= 0 too):
    perplexity exp(-mean log-prob), top-1 / top-5 accuracy from the ranks and, with `entropy` given, its mean in nats.
    -> dict(positions, perplexity, top1, top5, entropy or None)."""
    shapes = [tuple(token_logprobs.shape), tuple(rank.shape), tuple(ids.shape[:2])] + ([tuple(entropy.shape)] if entropy is not None else [])
    if len(ids.shape) != 3 or any(sh != shapes[0] for sh in shapes):
        raise ValueError('summary: token_logprobs %s, rank %s, ids %s%s do not describe the same positions'
                         % (shapes[0], shapes[1], tuple(ids.shape), ', entropy %s' % (shapes[3],) if entropy is not None else ''))
    ent = _rows(entropy) if entropy is not None else None
    n, s, t1, t5, h = 0, 0.0, 0, 0, 0.0
    for r, (lps, rks, row_ids) in enumerate(zip(_rows(token_logprobs), _rows(rank), _rows(ids))):
        for t, (lp, rk) in enumerate(zip(lps, rks)):
            if row_ids[t][0] < 0:
                continue
            n += 1
            s += float(lp)
            t1 += rk == 0
            t5 += 0 <= rk < 5
            if ent is not None:
                h += float(ent[r][t])
    if n == 0:
        raise ValueError('summary: no live position')
    return dict(positions=n, perplexity=math.exp(-s / n), top1=t1 / n, top5=t5 / n, entropy=h / n if ent is not None else None)


def uncertain(alts, token_logprobs, min_gap):
    """The positions at which the model's best alternative beats the scored word by more than `min_gap` nats:
    [(row, position, gap, best id)], in row / position order."""
    out = []
    for r, (ids, lps, rks, tls) in enumerate(zip(_rows(alts.ids), _rows(alts.logprobs), _rows(alts.rank), _rows(token_logprobs))):
        for t, rk in enumerate(rks):
            if rk < 0:
                continue
            gap = float(lps[t][0]) - float(tls[t])
            if gap > min_gap:
                out.append((r, t, gap, int(ids[t][0])))
    return out
