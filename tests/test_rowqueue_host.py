"""RowScheduler (radialog_amd/rowqueue.py) against a stub session: rows "finish" by EOS after scripted step counts. No GPU, no library.

The stub keeps its own per-row counters (slot, steps) the way the device does -- T at the refill, + 1 per step -- so the scheduler's host mirror is
checked against something it did not compute. Request i's prompt starts with the id 100 + i, which is how the stub knows whose script a row runs."""
import pytest
import torch

from radialog_amd.rowqueue import RowScheduler, chunked_steps

EOS, PAD = 2, 0


class StubSession:
    """eos_at[i]: request i emits EOS as its eos_at[i]-th token (1 = token 0); None = never. Token k of request i is 1000 * (i + 1) + k."""

    def __init__(self, rows, cap, max_len, eos_at, eos_id=EOS):
        self.rows, self.cap, self.max_len, self.eos_id, self.pad_id = rows, cap, max_len, eos_id, PAD
        self.eos_at = eos_at
        self.who = [None] * rows
        self.slot, self.steps, self.unf = [0] * rows, [0] * rows, [0] * rows
        self.tok = [[PAD] * cap for _ in range(rows)]
        self.log = []                      # ("refill", ids, mask, qf, rows) / ("step", n) / ("park", rows)
        self.total_steps = 0

    def _emit(self, r):
        i, k = self.who[r], self.steps[r]
        t = 1000 * (i + 1) + k
        if self.eos_id >= 0:
            if not self.unf[r]:
                t = PAD
            elif self.eos_at[i] is not None and k + 1 == self.eos_at[i]:
                t = self.eos_id
            if t == self.eos_id:
                self.unf[r] = 0
        if k < self.cap:
            self.tok[r][k] = t
        self.steps[r] = k + 1

    def refill(self, ids, mask, qf, rows):
        assert ids.shape == mask.shape and len(rows) == ids.shape[0] and len(set(rows)) == len(rows)
        assert ids.shape[1] + self.cap <= self.max_len
        self.log.append(("refill", ids.clone(), mask.clone(), None if qf is None else qf.clone(), list(rows)))
        for k, r in enumerate(rows):
            first = int(mask[k].nonzero()[0])
            assert bool((ids[k, :first] == PAD).all()) and bool((mask[k, first:] == 1).all())
            self.who[r] = int(ids[k, first]) - 100
            self.slot[r], self.steps[r], self.unf[r] = ids.shape[1], 0, 1
            self.tok[r] = [PAD] * self.cap
            self._emit(r)

    def step(self, n):
        self.log.append(("step", n))
        self.total_steps += n
        for _ in range(n):
            for r in range(self.rows):
                if self.who[r] is not None:
                    assert self.slot[r] < self.max_len, f"row {r} walked out of its cache row"
                    self.slot[r] += 1
                    self._emit(r)

    def poll(self):
        return [self.unf[r] if self.who[r] is not None else 0 for r in range(self.rows)], [self.steps[r] if self.who[r] is not None else 0 for r in range(self.rows)]

    def park(self, rows):
        self.log.append(("park", list(rows)))
        for r in rows:
            self.who[r], self.slot[r], self.steps[r], self.unf[r] = None, 0, 0, 0

    def read_tokens(self, row):
        return list(self.tok[row])


def _req(i, T, max_new, qf=False):
    ids = torch.arange(T, dtype=torch.int64) + 3
    ids[0] = 100 + i
    return (ids, torch.full((32, 8), float(i)) if qf else None, max_new)


def _expect(i, n, eos_at=None):
    out = [1000 * (i + 1) + k for k in range(n)]
    if eos_at is not None and eos_at <= n:
        out = out[:eos_at - 1] + [EOS]
    return out


def test_results_come_back_in_request_order_cut_at_eos_or_cap():
    caps = [5, 9, 3, 7, 4, 6]
    eos_at = [None, 4, None, None, 1, 20]          # request 1 ends by EOS at its 4th token, request 4 at token 0, request 5 never reaches its 20th
    reqs = [_req(i, 6 + i, caps[i]) for i in range(6)]
    ses = StubSession(rows=2, cap=max(caps), max_len=64, eos_at=eos_at)
    out = RowScheduler(ses, rows=2, stage=2, poll=4).run(reqs)
    assert [o.tolist() for o in out] == [_expect(i, caps[i], eos_at[i]) for i in range(6)]
    assert all(o.dtype == torch.int64 for o in out)


def test_a_refill_group_is_left_padded_to_its_longest_prompt_with_mask_and_pad_columns():
    reqs = [_req(0, 40, 4, qf=True), _req(1, 37, 4, qf=True), _req(2, 12, 4), _req(3, 33, 4, qf=True)]
    ses = StubSession(rows=4, cap=4, max_len=64, eos_at=[None] * 4)
    sch = RowScheduler(ses, rows=4, stage=4)
    sch.run(reqs)
    refills = [e for e in ses.log if e[0] == "refill"]
    # requests 0 and 1 share a prefill (both with an image); 2 has none and 3 has one again: three groups, queue order kept
    assert sch.groups == [[0, 1], [2], [3]] and [e[4] for e in refills] == [[0, 1], [2], [3]]
    _, ids, mask, qf, _ = refills[0]
    assert ids.shape == (2, 40) and ids.dtype == torch.int32 and mask.dtype == torch.int32
    assert ids[0].tolist() == reqs[0][0].tolist() and mask[0].tolist() == [1] * 40
    assert ids[1].tolist() == [PAD] * 3 + reqs[1][0].tolist() and mask[1].tolist() == [0] * 3 + [1] * 37
    assert qf.shape == (2, 32, 8) and qf[0, 0, 0] == 0.0 and qf[1, 0, 0] == 1.0
    assert refills[1][3] is None and refills[1][1].shape == (1, 12)
    assert sch.n_refills == 3 and sch.n_refill_rows == 4


def test_min_refill_waits_for_that_many_free_rows():
    caps = [2, 4, 6, 8, 3, 3, 3, 3]
    reqs = [_req(i, 8, caps[i]) for i in range(8)]

    def groups(min_refill):
        ses = StubSession(rows=4, cap=8, max_len=64, eos_at=[None] * 8, eos_id=-1)
        sch = RowScheduler(ses, rows=4, stage=4, poll=1, min_refill=min_refill)
        out = sch.run(reqs)
        assert [o.tolist() for o in out] == [_expect(i, caps[i]) for i in range(8)]
        return sch.groups, ses.total_steps
    g1, s1 = groups(1)
    g2, s2 = groups(2)
    # every freed row is refilled at once: row 0 after step 1 (request 4, done behind step 3, when row 1 ends too), row 2 behind step 5
    assert g1 == [[0, 1, 2, 3], [4], [5, 6], [7]]
    assert g2 == [[0, 1, 2, 3], [4, 5], [6, 7]]                # rows 0 and 1 wait for each other; the last two are all that is left
    assert s2 >= s1


def test_a_row_that_ends_by_eos_between_polls_is_cut_at_its_eos():
    # poll every 4 steps; request 0 emits EOS as its 3rd token: the poll behind step 4 finds the row finished, its tokens end at the EOS
    reqs = [_req(0, 8, 12), _req(1, 8, 12)]
    ses = StubSession(rows=2, cap=12, max_len=64, eos_at=[3, None])
    out = RowScheduler(ses, rows=2, stage=2, poll=4).run(reqs)
    assert out[0].tolist() == _expect(0, 12, 3) and len(out[0]) == 3 and out[1].tolist() == _expect(1, 12)
    assert ses.tok[0][3:] == [PAD] * 9 or ses.who[0] is None      # (the row emitted pads behind its EOS until it was parked)


def test_rows_are_parked_when_the_queue_is_empty_and_never_walk_out_of_the_cache():
    # one long request next to short ones: the rows of the short ones are parked once nothing waits, and the stub asserts slot < max_len at every step
    caps = [3, 40, 3]
    reqs = [_req(i, 8, caps[i]) for i in range(3)]
    ses = StubSession(rows=2, cap=40, max_len=48, eos_at=[None] * 3, eos_id=-1)
    sch = RowScheduler(ses, rows=2, stage=1, poll=4)
    out = sch.run(reqs)
    assert [len(o) for o in out] == caps
    parks = [e[1] for e in ses.log if e[0] == "park"]
    assert parks == [[0], [1]] or parks == [[0], [0, 1]] or sorted(sum(parks, [])) == [0, 1]
    assert ses.who == [None, None] and sch.parked == [True, True]


def test_capacity_is_refused_before_anything_runs():
    ses = StubSession(rows=2, cap=16, max_len=48, eos_at=[None] * 2)
    with pytest.raises(ValueError, match="exceeds max_len"):
        RowScheduler(ses, rows=2, stage=1).run([_req(0, 8, 4), _req(1, 40, 9)])       # 40 + 9 > 48
    with pytest.raises(ValueError, match="cap"):
        RowScheduler(ses, rows=2, stage=1).run([_req(0, 8, 17)])                      # more than the session's cap
    with pytest.raises(ValueError, match="cap"):
        RowScheduler(ses, rows=2, stage=1).run([_req(0, 36, 4)])                      # 36 + cap 16 > 48: a refill reserves cap slots
    with pytest.raises(ValueError, match="T >= 32"):
        RowScheduler(ses, rows=2, stage=1).run([_req(0, 8, 4, qf=True)])
    assert ses.log == []
    with pytest.raises(ValueError):
        RowScheduler(ses, rows=0, stage=1)


def test_the_host_mirror_follows_the_stubs_own_counters():
    caps = [5, 11, 7, 3, 9]
    reqs = [_req(i, 6 + 3 * i, caps[i]) for i in range(5)]

    class Checked(StubSession):
        sch = None

        def poll(self):
            for r in range(self.rows):
                if self.who[r] is not None:
                    assert (self.sch.slot[r], self.sch.steps[r]) == (self.slot[r], self.steps[r]), f"row {r}"
                    assert self.sch.req[r] == self.who[r]
            return super().poll()
    ses = Checked(rows=3, cap=11, max_len=64, eos_at=[None] * 5, eos_id=-1)
    sch = RowScheduler(ses, rows=3, stage=2, poll=3)
    ses.sch = sch
    out = sch.run(reqs)
    assert [len(o) for o in out] == caps
    assert sch.n_steps == ses.total_steps
    # a session that reports another count than the mirror holds is an error, not a silent cut
    bad = StubSession(rows=1, cap=4, max_len=64, eos_at=[None], eos_id=-1)
    bad.poll = lambda: ([1], [7])
    with pytest.raises(RuntimeError, match="mirror"):
        RowScheduler(bad, rows=1, stage=1).run([_req(0, 8, 4)])


# the request list of tests/test_gpu_rows.py's end-to-end leg: (T, max_new) per request, 4 rows
QUEUE_LIST = [(40, 4), (24, 12), (40, 5), (33, 3), (24, 10), (40, 4), (24, 3), (36, 11), (24, 4), (40, 6)]


def test_the_queue_takes_fewer_steps_than_the_chunked_schedule_on_the_gpu_tests_list():
    caps = [c for _, c in QUEUE_LIST]
    reqs = [_req(i, T, c) for i, (T, c) in enumerate(QUEUE_LIST)]
    ses = StubSession(rows=4, cap=max(caps), max_len=128, eos_at=[None] * len(reqs), eos_id=-1)
    sch = RowScheduler(ses, rows=4, stage=2, poll=4)
    out = sch.run(reqs)
    assert [len(o) for o in out] == caps
    assert chunked_steps(caps, 4) == (12 - 1) + (11 - 1) + (6 - 1)
    assert sch.n_steps < chunked_steps(caps, 4)


def test_generate_many_refuses_beams_rules_and_sampling():
    from radialog_amd.config import small_cfg
    from radialog_amd.modeling_llama_imgemb import LlamaForCausalLM
    m = LlamaForCausalLM(cfg=small_cfg().llama, max_batch=6, max_len=128)
    ids = [torch.arange(8) + 3]
    with pytest.raises(ValueError, match="num_beams"):
        m.generate_many(ids, num_beams=3)
    with pytest.raises(ValueError, match="sampling"):
        m.generate_many(ids, do_sample=True)
    for kw in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=3), dict(min_new_tokens=2)):
        with pytest.raises(ValueError, match="row session"):
            m.generate_many(ids, **kw)
    with pytest.raises(ValueError, match="max_new_tokens"):
        m.generate_many(ids, max_new_tokens=[3, 4])
    assert m._engine is None                   # nothing was built for a refused call
