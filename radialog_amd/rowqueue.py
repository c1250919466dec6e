"""Continuous batching on the host: a queue of waiting prompts over the live rows of one row session (include/rdx.h: rdx_rows_*).

`RowScheduler` is pure Python. It drives any object with the five methods of `RdxEngine.row_session(...)`:

    refill(ids [R, T] int, mask [R, T] int, qformer_embs [R, 32, D] or None, rows list[int])   R prompts into the listed live rows
    step(n)                 n decode steps of all rows (no sync)
    poll()                  -> (unfinished list[int], steps list[int]) per row, after draining the device
    park(rows list[int])    rows nobody uses
    read_tokens(row)        -> the row's generated tokens (a sequence of `cap` ints, pad_id behind the end)

and the attributes `cap` (tokens per request, max), `max_len`, `eos_id`, `pad_id`. The CPU tests run it against a stub with scripted row lengths.
"""
from __future__ import annotations

from collections import deque
from typing import List, Optional, Sequence, Tuple

import torch

Request = Tuple[torch.Tensor, Optional[torch.Tensor], int]      # (ids 1-D, qformer_embs [32, D] / [1, 32, D] or None, max_new)


def chunked_steps(caps: Sequence[int], rows: int) -> int:
    """Decode steps of the schedule without a queue: chunks of `rows` requests in order, each chunk one generate() with max_new = its largest cap
    (max_new - 1 steps behind the prefill, which selects token 0)."""
    caps = list(caps)
    return sum(max(caps[i:i + rows]) - 1 for i in range(0, len(caps), rows))


class RowScheduler:
    """Runs `requests` through the `rows` live rows of `session`, refilling a finished row from the queue while its neighbours go on decoding.

    stage: at most this many waiting prompts are prefilled together (one refill group, left-padded to its longest prompt). poll: decode steps between two
    looks at the rows (fewer when a request reaches its cap sooner). min_refill: a refill waits until this many rows are free -- fewer, larger prefills --
    unless fewer requests are waiting or no row is live.

    A request ends at EOS or at its own max_new; `run()` returns the generated tokens of every request, in request order, as 1-D int64 tensors cut there
    (the EOS included). The scheduler keeps the library's host mirror itself -- `slot[r]` = T of the refill + steps since, `steps[r]` = tokens selected -- and
    checks the step counts the poll reports against it."""

    def __init__(self, session, rows: int, stage: int, poll: int = 4, min_refill: int = 1):
        if rows < 1 or stage < 1 or poll < 1 or min_refill < 1:
            raise ValueError(f"rows ({rows}), stage ({stage}), poll ({poll}) and min_refill ({min_refill}) must be >= 1")
        self.s, self.rows, self.stage, self.poll, self.min_refill = session, rows, stage, poll, min(min_refill, rows)
        self.slot = [0] * rows             # host mirror: cache slot of the next token (0 = parked)
        self.steps = [0] * rows            # host mirror: tokens selected by the row's request so far
        self.req = [None] * rows           # index of the request a row is working on
        self.parked = [True] * rows        # a session starts with every row parked
        self.n_steps = 0                   # decode steps taken
        self.n_refills = 0                 # refill groups (one small prefill each)
        self.n_refill_rows = 0
        self.groups: List[List[int]] = []  # the request indices of every refill group, in order

    # ---------------------------------------------------------------------------------------------------------------
    def _check(self, requests: Sequence[Request]):
        cap, max_len = int(self.s.cap), int(self.s.max_len)
        for i, (ids, qf, max_new) in enumerate(requests):
            T = int(ids.numel())
            if ids.dim() != 1 or T < 1:
                raise ValueError(f"request {i}: ids must be a non-empty 1-D tensor")
            if max_new < 1:
                raise ValueError(f"request {i}: max_new must be positive, got {max_new}")
            if T + max_new > max_len:
                raise ValueError(f"request {i}: T ({T}) + max_new ({max_new}) exceeds max_len {max_len}")
            if max_new > cap:
                raise ValueError(f"request {i}: max_new {max_new} exceeds the session's cap {cap}")
            if T + cap > max_len:
                raise ValueError(f"request {i}: T ({T}) + the session's cap ({cap}) exceeds max_len {max_len} (a refill reserves cap slots behind the prompt)")
            if qf is not None and T < 32:
                raise ValueError(f"request {i}: the image splice needs T >= 32, got {T}")

    def _group(self, requests, waiting: deque, n: int) -> List[int]:
        """Up to n requests from the head of the queue that can share one prefill: all with image embeddings or all without."""
        first = requests[waiting[0]][1] is None
        group = []
        while waiting and len(group) < n and (requests[waiting[0]][1] is None) == first:
            group.append(waiting.popleft())
        return group

    def _refill(self, requests, group: List[int], rows: List[int]):
        pad = int(self.s.pad_id)
        T = max(int(requests[i][0].numel()) for i in group)
        ids = torch.full((len(group), T), pad, dtype=torch.int32)
        mask = torch.zeros((len(group), T), dtype=torch.int32)
        for k, i in enumerate(group):
            x = requests[i][0].to(device="cpu", dtype=torch.int32)
            ids[k, T - x.numel():] = x           # left-padded: the image splice position follows the pads, as in generate
            mask[k, T - x.numel():] = 1
        qf = None
        if requests[group[0]][1] is not None:
            qf = torch.stack([requests[i][1].reshape(requests[i][1].shape[-2], requests[i][1].shape[-1]).to(torch.float32).cpu() for i in group])
        self.s.refill(ids, mask, qf, list(rows))
        for r, i in zip(rows, group):
            self.req[r], self.slot[r], self.steps[r], self.parked[r] = i, T, 1, False
        self.n_refills += 1
        self.n_refill_rows += len(group)
        self.groups.append(list(group))

    def _finish(self, requests, results, r: int):
        i = self.req[r]
        max_new, eos = int(requests[i][2]), int(self.s.eos_id)
        toks = torch.as_tensor(self.s.read_tokens(r)).to(device="cpu", dtype=torch.int64).reshape(-1)[:min(self.steps[r], max_new)]
        if eos >= 0:
            hit = (toks == eos).nonzero()
            if hit.numel():
                toks = toks[:int(hit[0]) + 1]
        results[i] = toks.clone()
        self.req[r] = None

    # ---------------------------------------------------------------------------------------------------------------
    def run(self, requests: Sequence[Request]) -> List[torch.Tensor]:
        requests = list(requests)
        self._check(requests)                  # before anything runs
        results: List[Optional[torch.Tensor]] = [None] * len(requests)
        waiting = deque(range(len(requests)))
        while True:
            free = [r for r in range(self.rows) if self.req[r] is None]
            live = self.rows - len(free)
            # refill: as many groups as there are free rows and waiting prompts, once enough rows are free
            if waiting and free and (len(free) >= min(self.min_refill, len(waiting)) or live == 0):
                while waiting and free:
                    group = self._group(requests, waiting, min(self.stage, len(free)))
                    self._refill(requests, group, free[:len(group)])
                    free = free[len(group):]
            # rows that stay free run parked (no token written, no walk out of the cache row)
            idle = [r for r in free if not self.parked[r]]
            if idle:
                self.s.park(idle)
                for r in idle:
                    self.slot[r], self.steps[r], self.parked[r] = 0, 0, True
            busy = [r for r in range(self.rows) if self.req[r] is not None]
            if not busy:
                break
            # a request whose cap is already reached (max_new == 1: token 0 is all of it) needs no step
            left = min(int(requests[self.req[r]][2]) - self.steps[r] for r in busy)
            if left > 0:
                n = min(self.poll, left)
                self.s.step(n)
                self.n_steps += n
                for r in busy:
                    self.slot[r] += n
                    self.steps[r] += n
            unf, steps = self.s.poll()
            for r in busy:
                if int(steps[r]) != self.steps[r]:
                    raise RuntimeError(f"row {r}: the session reports {int(steps[r])} tokens, the scheduler's mirror holds {self.steps[r]}")
                if not int(unf[r]) or self.steps[r] >= int(requests[self.req[r]][2]):
                    self._finish(requests, results, r)
        return results
