"""Host restatement of prompt-lookup decoding (include/rdx.h: rdx_generate_lookup; the kernel: radialog_amd/csrc/lookup.hip), in plain Python lists.

The draft rule. H = corpus + prompt ids as passed + every emitted token. For n = ngram_max down to ngram_min: among the starts j with H[j : j + n] equal to
the last n tokens of H and j + n < len(H), the largest; the draft is H[j + n : min(j + n + draft_len, len(H))]. The first n with a match wins.
The draft is clipped so that a pass never emits beyond max_new (d <= max_new - emitted - 1) and never writes a cache slot at or beyond T + max_new.
Given the emitted sequence S, the accepted count of a forward is the longest draft prefix equal to S's continuation; the forward emits those and one more
token, unless an EOS among them ends the emission (and the call)."""
from dataclasses import dataclass
from typing import List, Sequence, Tuple


@dataclass(frozen=True)
class Rule:
    draft_len: int = 8
    ngram_max: int = 3
    ngram_min: int = 1


def find_draft(H: Sequence[int], limit: int, ngram_max: int, ngram_min: int) -> List[int]:
    """The draft for the sequence H, at most `limit` tokens long ([]: no match, or limit <= 0)."""
    if limit <= 0:
        return []
    L = len(H)
    for n in range(ngram_max, ngram_min - 1, -1):
        if n >= L:
            continue
        pat = list(H[L - n:])
        for j in range(L - n - 1, -1, -1):                   # j + n < L, the largest first
            if list(H[j:j + n]) == pat:
                return list(H[j + n:min(j + n + limit, L)])
    return []


def draft_limit(rule: Rule, emitted: int, max_new: int, slot: int, slot_end: int) -> int:
    """How long the next draft may be: the rule's length, the tokens still to emit minus the pass's own, the call's cache slots behind `slot`."""
    return max(0, min(rule.draft_len, max_new - emitted - 1, slot_end - 1 - slot))


def simulate(prompt: Sequence[int], corpus: Sequence[int], S: Sequence[int], rule: Rule, max_new: int, eos_id: int = -1) -> Tuple[List[Tuple[int, int]], dict]:
    """The (drafted, accepted) trace of every forward behind the prompt and the stats of a call that emitted exactly S (EOS included, pads not)."""
    S = list(S)
    T = len(prompt)
    assert 1 <= len(S) <= max_new
    H = list(corpus) + list(prompt) + [S[0]]
    emitted = 1
    done = (eos_id >= 0 and S[0] == eos_id) or emitted >= max_new
    trace = []
    while not done:
        assert emitted < len(S), "S ends before the call would have"
        slot = T + emitted - 1                               # the slot the next forward's first row is written to
        dr = find_draft(H, draft_limit(rule, emitted, max_new, slot, T + max_new), rule.ngram_max, rule.ngram_min)
        a = 0
        while a < len(dr) and emitted + a < len(S) and dr[a] == S[emitted + a]:
            a += 1
        n = 0
        for j in range(a + 1):
            assert emitted + j < len(S), "S ends inside a forward"
            n = j + 1
            if eos_id >= 0 and S[emitted + j] == eos_id:
                done = True
                break
        H += S[emitted:emitted + n]
        emitted += n
        done = done or emitted >= max_new
        trace.append((len(dr), a))
    assert emitted == len(S), f"the call would have emitted {emitted} tokens, S holds {len(S)}"
    stats = {"passes": sum(1 for d, _ in trace if d > 0), "drafted": sum(d for d, _ in trace), "accepted": sum(a for d, a in trace if d > 0),
             "forwards": len(trace)}
    return trace, stats


def accept_step(am: Sequence[int], tail: Sequence[int], state: Sequence[int], hist: Sequence[int], corpus: Sequence[int], rule: Rule, max_new: int,
                slot_end: int, eos_id: int = -1, pad_id: int = 0, advance: bool = True):
    """One launch of lookup_accept_k restated: am = the argmax of each of the d + 1 rows, tail = [last token, draft_1 .. draft_d], state = (step, slot,
    position, unfinished), hist = the history so far. Returns a dict: emitted tokens, accepted (as traced), state, hist, the next tail, finished."""
    d = len(tail) - 1
    step, slot, pos, unf = state
    acc = 0
    while acc < d and am[acc] == tail[acc + 1]:
        acc += 1
    if eos_id < 0:
        unf = 1
    hist = list(hist)
    out, cut = [], False
    for j in range(acc + 1):
        tok = am[j] if unf else pad_id
        if eos_id >= 0 and tok == eos_id:
            unf = 0
        out.append(tok)
        hist.append(tok)
        if not unf:
            cut = j < acc
            break
    n = len(out)
    if advance:
        slot, pos = slot + n, pos + n
    step += n
    fin = (not unf) or step >= max_new
    limit = 0 if fin else draft_limit(rule, step, max_new, slot, slot_end)
    dr = find_draft(list(corpus) + hist, limit, rule.ngram_max, rule.ngram_min)
    return {"emitted": out, "accepted": n if cut else acc, "state": (step, slot, pos, int(bool(unf))), "hist": hist, "tail": [out[-1]] + dr,
            "finished": bool(fin), "eos": not unf}
