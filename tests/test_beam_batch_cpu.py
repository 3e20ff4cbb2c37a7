"""CPU: the host half of the batched beam search (beam.rebuild_hypotheses) on hand-written trellises, against a straight
Python transcription of beam.py's per-step list bookkeeping (live / nxt / final, stable sorts)."""
import importlib
import numpy as np
import pytest


@pytest.fixture(scope='module')
def bm():
    importlib.import_module('end-to-end-asr-pytorch_amd')
    return importlib.import_module('end-to-end-asr-pytorch_amd.beam')


def f32(v):
    return float(np.float32(v))


def bookkeeping(tables, beam, steps):
    """beam.py:92-172 with the device taken out: tables[t][slot] is that live hypothesis' top-k list [(token, score)]."""
    live = [([], [], 0)]
    final = []
    for t in range(steps):
        nxt = []
        for seq, scores, n in live:
            term = None
            for tk, sc in tables[t][n]:
                sc = f32(sc)
                if tk == 1:
                    term = sc
                    continue
                nxt.append((seq + [tk], scores + [sc], n))
            if term is not None:
                final.append((seq + [1], scores + [term]))
                if beam == 1:
                    return final
        nxt.sort(key=lambda o: sum(o[1]) / len(o[1]), reverse=True)
        nxt = nxt[:beam]
        live = []
        if not nxt:
            break
        live = [(seq, scores, slot) for slot, (seq, scores, _) in enumerate(nxt)]
    final += [(seq, scores) for seq, scores, _ in live]
    final.sort(key=lambda o: sum(o[1]) / len(o[1]), reverse=True)
    return final[:beam]


def write_trellis(bm, tables_per_utt, beam, steps):
    """What las_beam_select records (include/las_hip.h), written by hand-rolled Python: per step and utterance the new slots'
    (token, parent, score), the old slots' (terminated, score) and the new live count; -1 past an utterance's limit."""
    U, R = len(tables_per_utt), len(tables_per_utt) * beam
    S = max(steps)
    tr = np.zeros((S, bm.trellis_words(U, beam)), dtype=np.int32)
    fl = tr.view(np.float32)
    for u, tables in enumerate(tables_per_utt):
        state = [(0.0, 0)]                                  # per live slot: fp64 running sum, prefix length
        r0 = u * beam
        for t in range(S):
            if t >= steps[u]:
                tr[t, 5 * R + u] = -1
                continue
            cands = []
            for s, (sm, ln) in enumerate(state):
                for tk, sc in tables[t][s] if t < len(tables) and s < len(tables[t]) else []:
                    if tk == 1:
                        tr[t, 3 * R + r0 + s] = 1
                        fl[t, 4 * R + r0 + s] = sc
                    else:
                        cands.append(((sm + f32(sc)) / (ln + 1), s, tk, sc, sm + f32(sc), ln + 1))
            order = sorted(range(len(cands)), key=lambda i: (-cands[i][0], i))[:beam]
            state = []
            for slot, i in enumerate(order):
                _, s, tk, sc, sm, ln = cands[i]
                tr[t, r0 + slot], tr[t, R + r0 + slot], fl[t, 2 * R + r0 + slot] = tk, s, sc
                state.append((sm, ln))
            tr[t, 5 * R + u] = len(state)
    return tr


def same(hyps, want):
    assert len(hyps) == len(want)
    for h, (seq, scores) in zip(hyps, want):
        assert h.outIndex == seq
        assert h.output_scores == scores              # the same float32 values, exactly


# utterance A, beam 2; a step's table is [slot] -> that hypothesis' top-k list
A = [
    [[(4, -0.1), (5, -0.9)]],                                   # step 0: one empty hypothesis
    [[(6, -0.2), (1, -0.3)], [(1, -0.05), (7, -2.0)]],          # step 1: both slots see <eos> (terminate in slot order)
    [[(8, -0.4), (9, -0.5)], [(1, -0.1), (2, -0.6)]],           # step 2: slot 1 terminates
    [[(3, -0.3), (1, -0.2)], [(2, -0.1), (3, -0.7)]],           # step 3
]
# utterance B, beam 2: the two candidates of step 1 tie in average score exactly -> the earlier one ranks first
B = [
    [[(4, -0.5), (5, -0.5)]],
    [[(6, -0.25), (7, -0.75)], [(8, -0.25), (9, -1.0)]],
    [[(2, -0.5)], [(2, -0.5)]],
]


def test_termination_at_several_steps(bm):
    tr = write_trellis(bm, [A], 2, [4])
    got = bm.rebuild_hypotheses(tr, 1, 2, [4])
    want = bookkeeping(A, 2, 4)
    same(got[0], want)
    assert sum(h.outIndex[-1] == 1 for h in got[0]) >= 1       # a terminated hypothesis made the list


def test_literal_trellis(bm):
    """A trellis typed in word by word (U=1, beam=2, 2 steps) and the list it must give."""
    R = 2
    tr = np.zeros((2, bm.trellis_words(1, 2)), dtype=np.int32)
    fl = tr.view(np.float32)
    tr[0, 0:2] = [4, 5]; tr[0, R:R + 2] = [0, 0]; fl[0, 2 * R:2 * R + 2] = [-0.1, -0.9]; tr[0, 5 * R] = 2
    tr[1, 0:2] = [6, 7]; tr[1, R:R + 2] = [0, 1]; fl[1, 2 * R:2 * R + 2] = [-0.2, -2.0]
    tr[1, 3 * R:3 * R + 2] = [1, 1]; fl[1, 4 * R:4 * R + 2] = [-0.3, -0.05]; tr[1, 5 * R] = 2
    got = bm.rebuild_hypotheses(tr, 1, 2, [2])[0]
    # final = [4,1] (avg -0.2), [5,1] (avg -0.475), then survivors [4,6] (avg -0.15), [5,7] (avg -1.45)
    assert [h.outIndex for h in got] == [[4, 6], [4, 1]]
    assert got[0].output_scores == [f32(-0.1), f32(-0.2)] and got[1].output_scores == [f32(-0.1), f32(-0.3)]


def test_tie_resolved_by_order(bm):
    tr = write_trellis(bm, [B], 2, [3])
    got = bm.rebuild_hypotheses(tr, 1, 2, [3])
    want = bookkeeping(B, 2, 3)
    same(got[0], want)
    # step 1: [4,6] and [5,8] both average (-0.5-0.25)/2; the one expanded first (parent slot 0) must come first
    assert got[0][0].outIndex[:2] == [4, 6] and got[0][1].outIndex[:2] == [5, 8]
    assert got[0][0].avgScore() == got[0][1].avgScore()


def test_beam1_early_end(bm):
    G = [[[(4, -0.1)]], [[(5, -0.2)]], [[(1, -0.3)]], [[(6, -0.1)]]]
    tr = write_trellis(bm, [G], 1, [4])
    got = bm.rebuild_hypotheses(tr, 1, 1, [4])
    want = bookkeeping(G, 1, 4)
    assert want == [([4, 5, 1], [f32(-0.1), f32(-0.2), f32(-0.3)])]
    same(got[0], want)
    G2 = [[[(4, -0.1)]], [[(5, -0.2)]]]                          # no <eos> within the limit: the survivor is returned
    same(bm.rebuild_hypotheses(write_trellis(bm, [G2], 1, [2]), 1, 1, [2])[0], bookkeeping(G2, 1, 2))


def test_every_candidate_is_eos(bm):
    G = [[[(4, -0.1), (1, -0.2)]], [[(1, -0.3)]], [[(5, -0.1)]]]   # step 1: nxt is empty, the loop breaks
    tr = write_trellis(bm, [G], 2, [3])
    same(bm.rebuild_hypotheses(tr, 1, 2, [3])[0], bookkeeping(G, 2, 3))


def test_mixed_batch_with_shorter_limit(bm):
    """Three utterances in one trellis; the middle one's step limit (2) is shorter than the batch's (4)."""
    steps = [4, 2, 3]
    tr = write_trellis(bm, [A, A, B], 2, steps)
    assert tr[2, 5 * 6 + 1] == -1 and tr[3, 5 * 6 + 2] == -1
    got = bm.rebuild_hypotheses(tr, 3, 2, steps)
    same(got[0], bookkeeping(A, 2, 4))
    same(got[1], bookkeeping(A, 2, 2))
    same(got[2], bookkeeping(B, 2, 3))
    assert [h.outIndex for h in got[1]] != [h.outIndex for h in got[0]]


def test_random_tables(bm):
    rng = np.random.RandomState(0)
    for beam, kb, S in [(3, 3, 6), (5, 4, 8), (1, 1, 5), (4, 2, 7)]:
        utts, steps = [], []
        for u in range(4):
            tabs = []
            for t in range(S):
                tabs.append([[(int(tk), float(np.round(-rng.rand(), 1))) for tk in rng.permutation(7)[:kb]] for _ in range(beam)])
            utts.append(tabs)
            steps.append(int(rng.randint(1, S + 1)))
        tr = write_trellis(bm, utts, beam, steps)
        got = bm.rebuild_hypotheses(tr, 4, beam, steps)
        for u in range(4):
            same(got[u], bookkeeping(utts[u], beam, steps[u]))
