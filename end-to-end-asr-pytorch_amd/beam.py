"""Joint CTC/attention beam search (reference src/asr.py:155-258 `Seq2Seq.beam_decode`, src/ctc.py `CTCPrefixScore`,
src/postprocess.py:44-119 `Hypothesis`), with every hypothesis of the beam advanced in ONE batched decode step on the
device: the decoder step kernels run with batch = live hypotheses, the CTC prefix scorer with one thread per
(hypothesis, candidate) pair.  The host keeps the reference's bookkeeping (expansion, <eos> handling, average-score
ranking) on the few numbers it needs per step: the top-k scores/ids and the candidate lists.
"""
import ctypes
import torch

from . import _lib, ops
from ._lib import P, I, F, ptr, check, cur_stream
from .decoder import DecDims, DecState, make_params, weight_names, s_dtype, LOC_C

CTC_BEAM_RATIO = 1.5          # asr.py:15


class Hypothesis:
    """Result record with the reference's accessors (postprocess.py:48-119)."""

    def __init__(self, seq, scores):
        self.output_seq, self.output_scores = list(seq), list(scores)

    def avgScore(self):
        assert len(self.output_scores) != 0
        return sum(self.output_scores) / len(self.output_scores)

    @property
    def outIndex(self):
        return [int(i) for i in self.output_seq]


class _Live:
    __slots__ = ('seq', 'scores', 'slot')

    def __init__(self, seq, scores, slot):
        self.seq, self.scores, self.slot = seq, scores, slot          # slot: row of the device state tensors

    def avg(self):
        return sum(self.scores) / len(self.scores)


def beam_decode(model, audio_feature, decode_step, state_len, decode_beam_size):
    """Returns the top `decode_beam_size` Hypothesis objects of ONE utterance (asr.py:155-258)."""
    L_ = _lib.lib()
    assert audio_feature.shape[0] == 1
    if getattr(model, 'decode_lm_weight', 0) > 0:
        raise NotImplementedError('RNN-LM fusion (asr.py:232-235) is outside the LAS path (SURVEY.md §2.1)')
    if not model.joint_att:
        return []                                      # as the reference: nothing is decoded without the attention decoder
    beam = int(decode_beam_size)
    dev = audio_feature.device
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.no_grad():
        lens_host = [int(v) for v in state_len]
        lens_dev = torch.tensor(lens_host, **i32)
        enc, enc_len_dev, enc_len = model.encode(audio_feature.float(), lens_dev, lens_host)
        enc = enc.contiguous()
        Tp, E = int(enc.shape[1]), int(enc.shape[2])
        if decode_step == 0:
            decode_step = int(enc_len[0])
        V, C, NL, A = model.char_dim, model.dec_dim, model.dec_layers, model.A
        loc = model.att_mode == 'loc'
        lam = float(model.ctc_weight)
        joint_ctc = bool(model.joint_ctc)
        K = min(int(CTC_BEAM_RATIO * beam), V)
        kb = min(beam, V)
        names = weight_names(NL, loc)
        W = {n: model.P(n).detach().contiguous() for n in names}
        params = make_params(W, NL, loc)
        psi = ops.linear(enc, model.P('attention.psi.weight'), model.P('attention.psi.bias'), act=1).contiguous()
        lp = r_prev = None
        if joint_ctc:
            logit = ops.linear(enc, model.P('ctc_layer.weight'), model.P('ctc_layer.bias'))[0].contiguous()     # [T',V]
            lp = torch.empty_like(logit)
            check(L_.las_log_softmax_rows(ptr(logit), I(Tp), I(V), ptr(lp), cur_stream()), 'las_log_softmax_rows')
            r_prev = torch.empty(1, Tp, 2, **f32)
            check(L_.las_ctc_prefix_init(ptr(lp), I(Tp), I(V), ptr(r_prev), cur_stream()), 'las_ctc_prefix_init')
        # the utterance's encoding, replicated once for the widest beam (the step kernels index enc/psi per hypothesis)
        encB = enc.expand(beam, Tp, E).contiguous()
        psiB = psi.expand(beam, Tp, A).contiguous()
        lenB = enc_len_dev.expand(beam).contiguous()
        # device state of the live hypotheses (row = hypothesis)
        h = torch.zeros(NL, 1, C, **f32)
        c = torch.zeros(NL, 1, C, **f32)
        att = torch.zeros(1, Tp, **f32)
        if loc:
            att[0, :enc_len[0]] = 1.0 / enc_len[0]                     # Attention.forward's first-call init (asr.py:444-449)
        tok = torch.zeros(1, **i32)
        plen = torch.zeros(1, **i32)
        prev_ctc = torch.zeros(1, **f32)
        live = [_Live([], [], 0)]
        final = []
        for t in range(decode_step):
            N = len(live)
            d = DecDims(N, Tp, E, A, C, NL, V, 1, int(loc), ops._prec)
            hs = torch.empty(NL, 2, N, C, **f32)
            cs = torch.empty(NL, 2, N, C, **f32)
            hs[:, 0] = h
            cs[:, 0] = c
            attb = torch.empty(2, N, Tp, **f32)
            attb[0] = att
            S = dict(tok=tok.contiguous(), xin=torch.empty(1, N, C + E, **f32), q=torch.empty(1, N, A, **f32), att=attb, hs=hs,
                     cs=cs, gates=torch.empty(NL, 1, N, 4 * C, **f32), ebuf=torch.empty(N, Tp, **f32),
                     logits_step=torch.empty(N, V, **f32))
            if loc:
                S['f'] = torch.empty(1, N, LOC_C, Tp, **f32)
                S['s'] = torch.empty(1, N, Tp, A, dtype=s_dtype(d.prec), device=dev)
            st = DecState()
            for k, v in S.items():
                setattr(st, k, v.data_ptr())
            logits = torch.empty(N, V, **f32)
            check(L_.las_decoder_step(ctypes.byref(d), ctypes.byref(params), ptr(encB), ptr(psiB), ptr(lenB), ctypes.byref(st),
                                      ptr(logits), cur_stream()), 'las_decoder_step')
            cur = torch.empty_like(logits)
            check(L_.las_log_softmax_rows(ptr(logits), I(N), I(V), ptr(cur), cur_stream()), 'las_log_softmax_rows')
            cand = psi_c = r_out = None
            if joint_ctc:
                cv = torch.empty(N, K, **f32)
                cand = torch.empty(N, K, **i32)
                check(L_.las_topk_rows(ptr(cur), I(N), I(V), I(K), ptr(cv), ptr(cand), cur_stream()), 'las_topk_rows')
                psi_c = torch.empty(N, K, **f32)
                r_out = torch.empty(N, K, Tp, 2, **f32)
                check(L_.las_ctc_prefix_score(ptr(lp), I(Tp), I(V), ptr(r_prev), ptr(tok), ptr(plen), ptr(cand), I(N), I(K),
                                              ptr(psi_c), ptr(r_out), cur_stream()), 'las_ctc_prefix_score')
                check(L_.las_beam_combine(ptr(cur), I(N), I(V), ptr(cand), ptr(psi_c), ptr(prev_ctc), I(K), F(lam),
                                          cur_stream()), 'las_beam_combine')
            topv = torch.empty(N, kb, **f32)
            topi = torch.empty(N, kb, **i32)
            check(L_.las_topk_rows(ptr(cur), I(N), I(V), I(kb), ptr(topv), ptr(topi), cur_stream()), 'las_topk_rows')
            # ---- host bookkeeping on N x beam numbers (Hypothesis.addTopk, postprocess.py:71-104)
            pack = [topv, topi.float()] + ([cand.float()] if joint_ctc else [])       # one D2H (ids < 2^24 are exact in fp32)
            host = torch.cat(pack, dim=1).cpu()
            topv_h = host[:, :kb].tolist()
            topi_h = host[:, kb:2 * kb].to(torch.int64).tolist()
            cand_h = host[:, 2 * kb:].to(torch.int64).tolist() if joint_ctc else None
            nxt = []
            for hyp in live:
                n = hyp.slot
                term = None
                for i in range(kb):
                    tk, sc = int(topi_h[n][i]), float(topv_h[n][i])
                    if tk == 1:
                        term = sc
                        continue
                    j = cand_h[n].index(tk) if joint_ctc else 0
                    nxt.append((_Live(hyp.seq + [tk], hyp.scores + [sc], None), n, j))
                if term is not None:
                    final.append(Hypothesis(hyp.seq + [1], hyp.scores + [term]))
                    if beam == 1:
                        return final
            nxt.sort(key=lambda o: o[0].avg(), reverse=True)            # stable, as list.sort in the reference
            nxt = nxt[:beam]
            live = []
            if not nxt:
                break
            parents = torch.tensor([p for _, p, _ in nxt], dtype=torch.long, device=dev)
            h = hs[:, 1].index_select(1, parents)
            c = cs[:, 1].index_select(1, parents)
            att = attb[1].index_select(0, parents)
            tok = torch.tensor([o.seq[-1] for o, _, _ in nxt], **i32)
            plen = torch.tensor([len(o.seq) for o, _, _ in nxt], **i32)
            if joint_ctc:
                js = torch.tensor([j for _, _, j in nxt], dtype=torch.long, device=dev)
                r_prev = r_out[parents, js].contiguous()
                prev_ctc = psi_c[parents, js].contiguous()
            for slot, (o, _, _) in enumerate(nxt):
                o.slot = slot
                live.append(o)
        final += [Hypothesis(o.seq, o.scores) for o in live]
        final.sort(key=lambda o: o.avgScore(), reverse=True)
        return final[:beam]


# ---------------------------------------------------------------------------------------------------------------------
# Batched decoding: U utterances per call, the beam loop kept on the device (las_beam_select / las_beam_gather).  Rows of
# every per-step tensor are r = u*beam + slot; the host enqueues the whole loop and reads one trellis back at the end.

ENC_REPLICA_BUDGET = 1 << 30      # bytes of per-row enc + psi replicas (U*beam*T'*(E+A)*4) one batch may hold; more is split
STEP_ROWS = 128                   # rows one las_decoder_step call takes (the skinny products tile <= 128 batch rows)


def trellis_words(U, beam):
    """32-bit words of one step's trellis record (las_beam_select's `rec`)."""
    return 5 * U * beam + U


def rebuild_hypotheses(trellis, U, beam, steps):
    """Host half of the batched beam search; needs no GPU.  trellis: int32 array [S][trellis_words(U, beam)] as written by
    las_beam_select (float fields as their bit patterns), steps: per-utterance step limits.  Replays the reference's list
    bookkeeping (asr.py:237-258): `final` in the order hypotheses terminated (step, then slot), then the survivors, a
    stable sort by average score, the first `beam`.  Returns list[list[Hypothesis]]."""
    import numpy as np
    tr = np.ascontiguousarray(np.asarray(trellis, dtype=np.int32)).reshape(-1, trellis_words(U, beam))
    R = U * beam
    tok, par = tr[:, 0:R], tr[:, R:2 * R]
    score = tr[:, 2 * R:3 * R].view(np.float32)
    term = tr[:, 3 * R:4 * R]
    tscore = tr[:, 4 * R:5 * R].view(np.float32)
    cnt = tr[:, 5 * R:]
    out = []
    for u in range(U):
        live = [([], [])]
        final = []
        r0 = u * beam
        ended = False
        for t in range(int(steps[u])):
            for s, (seq, scores) in enumerate(live):
                if term[t, r0 + s]:
                    final.append(Hypothesis(seq + [1], scores + [float(tscore[t, r0 + s])]))
                    if beam == 1:
                        ended = True              # asr.py:246-247: returns `final` as it is
                        break
            if ended:
                break
            n = int(cnt[t, u])
            live = [(live[int(par[t, r0 + i])][0] + [int(tok[t, r0 + i])],
                     live[int(par[t, r0 + i])][1] + [float(score[t, r0 + i])]) for i in range(n)]
            if not live:
                break
        if ended:
            out.append(final)
            continue
        final += [Hypothesis(seq, scores) for seq, scores in live]
        final.sort(key=lambda o: o.avgScore(), reverse=True)
        out.append(final[:beam])
    return out


def _encode_batch(model, x, lens_host):
    """enc [U][T'max][E] (zero beyond each utterance's frames for VGG, the packed recurrence's padding otherwise) and the
    encoded lengths.  A BiRNN encoder runs the batch at once: the packed recurrence gives every utterance the frames it
    gets alone.  A VGG front-end does not (bias + ReLU make padded frames non-zero and the next conv reads them), so those
    utterances are encoded one by one, trimmed to their own length."""
    dev = x.device
    i32 = dict(dtype=torch.int32, device=dev)
    if not model.vgg:
        enc, enc_len_dev, enc_len = model.encode(x, torch.tensor(lens_host, **i32), lens_host)
        return enc.contiguous(), enc_len_dev.to(torch.int32).contiguous(), [int(v) for v in enc_len]
    encs, enc_len = [], []
    for u, n in enumerate(lens_host):
        e, _, el = model.encode(x[u:u + 1, :n].contiguous(), torch.tensor([n], **i32), [n])
        encs.append(e[0])
        enc_len.append(int(el[0]))
    Tp = max(e.shape[0] for e in encs)
    enc = torch.zeros(len(encs), Tp, encs[0].shape[1], dtype=torch.float32, device=dev)
    for u, e in enumerate(encs):
        enc[u, :e.shape[0]] = e
    return enc, torch.tensor(enc_len, **i32), enc_len


def max_batch(model, beam, max_len):
    """Largest U one device loop takes: U*beam rows within STEP_ROWS and the per-row enc + psi replicas within
    ENC_REPLICA_BUDGET for utterances of up to max_len frames."""
    if beam > STEP_ROWS:
        raise _lib.LasError(f'beam {beam} exceeds the {STEP_ROWS} rows of one decode step')
    red = 4 if model.vgg else 1
    for sr in model.srs:
        red *= sr
    Tp = max(1, max_len // red)
    per_utt = beam * Tp * (model.enc_out_dim + model.A) * 4
    return max(1, min(ENC_REPLICA_BUDGET // per_utt, STEP_ROWS // beam))


def beam_decode_batch(model, audio_feature, decode_steps, state_len, decode_beam_size):
    """Top `decode_beam_size` hypotheses of each of the U utterances of audio_feature [U,T,D] (asr.py:155-258 per utterance):
    list[list[Hypothesis]].  decode_steps: int or one per utterance, 0 = that utterance's encoded length."""
    U = int(audio_feature.shape[0])
    if getattr(model, 'decode_lm_weight', 0) > 0:
        raise NotImplementedError('RNN-LM fusion (asr.py:232-235) is outside the LAS path (SURVEY.md §2.1)')
    if not model.joint_att:
        return [[] for _ in range(U)]
    lens_host = [int(v) for v in state_len]
    assert len(lens_host) == U and min(lens_host) > 0
    steps = [int(decode_steps)] * U if isinstance(decode_steps, int) else [int(v) for v in decode_steps]
    assert len(steps) == U
    cap = max_batch(model, int(decode_beam_size), max(lens_host))
    cap = -(-U // -(-U // cap))                       # a larger request: several device loops of (nearly) equal size
    out = []
    for b in range(0, U, cap):
        out += _decode_chunk(model, audio_feature[b:b + cap], steps[b:b + cap], lens_host[b:b + cap], int(decode_beam_size))
    return out


def _decode_chunk(model, x, steps, lens_host, beam):
    L_ = _lib.lib()
    U = int(x.shape[0])
    dev = x.device
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.no_grad():
        x = x[:, :max(lens_host)].float().contiguous()
        enc, enc_len_dev, enc_len = _encode_batch(model, x, lens_host)
        Tp, E = int(enc.shape[1]), int(enc.shape[2])
        steps = [s if s > 0 else enc_len[u] for u, s in enumerate(steps)]
        S = max(steps)
        V, C, NL, A = model.char_dim, model.dec_dim, model.dec_layers, model.A
        loc = model.att_mode == 'loc'
        lam = float(model.ctc_weight)
        joint_ctc = bool(model.joint_ctc)
        K = min(int(CTC_BEAM_RATIO * beam), V)
        kb = min(beam, V)
        R = U * beam
        names = weight_names(NL, loc)
        W = {n: model.P(n).detach().contiguous() for n in names}
        params = make_params(W, NL, loc)
        psi = ops.linear(enc, model.P('attention.psi.weight'), model.P('attention.psi.bias'), act=1).contiguous()
        # ---- everything the loop touches is allocated here, once
        r_prev = prev_ctc = lp = cv = cand = psi_c = r_out = None
        if joint_ctc:
            logit = ops.linear(enc, model.P('ctc_layer.weight'), model.P('ctc_layer.bias')).contiguous()          # [U,T',V]
            lp = torch.empty_like(logit)
            check(L_.las_log_softmax_rows(ptr(logit), I(U * Tp), I(V), ptr(lp), cur_stream()), 'las_log_softmax_rows')
            r0 = torch.zeros(U, Tp, 2, **f32)
            check(L_.las_ctc_prefix_init_batch(ptr(lp), I(U), I(Tp), I(V), ptr(enc_len_dev), ptr(r0), cur_stream()),
                  'las_ctc_prefix_init_batch')
            r_prev = torch.zeros(U, beam, Tp, 2, **f32)
            r_prev[:, 0] = r0
            prev_ctc = torch.zeros(R, **f32)
            cv = torch.zeros(R, K, **f32)
            cand = torch.zeros(R, K, **i32)
            psi_c = torch.zeros(R, K, **f32)
            r_out = torch.zeros(R, K, Tp, 2, **f32)
        encB = enc.repeat_interleave(beam, 0).contiguous()             # las_decoder_step indexes enc / psi per row
        psiB = psi.repeat_interleave(beam, 0).contiguous()
        lenB = enc_len_dev.repeat_interleave(beam).contiguous()
        row_utt = torch.arange(U, **i32).repeat_interleave(beam).contiguous()
        limit = torch.tensor(steps, **i32)
        hs = torch.zeros(NL, 2, R, C, **f32)                            # slot 0: state the step reads, slot 1: what it writes
        cs = torch.zeros(NL, 2, R, C, **f32)
        attb = torch.zeros(2, R, Tp, **f32)
        if loc:                                                         # Attention.forward's first-call init (asr.py:444-449)
            inv = torch.tensor([1.0 / n for n in enc_len], **f32)
            mask = torch.arange(Tp, device=dev)[None, :] < enc_len_dev[:, None]
            attb[0] = (mask.float() * inv[:, None]).repeat_interleave(beam, 0)
        tok = torch.zeros(R, **i32)
        plen = torch.zeros(R, **i32)
        ssum = torch.zeros(R, dtype=torch.float64, device=dev)
        n_live = torch.ones(U, **i32)                                   # one empty hypothesis per utterance, in slot 0
        parent, tok_n, j_n, plen_n = (torch.zeros(R, **i32) for _ in range(4))
        sum_n = torch.zeros(R, dtype=torch.float64, device=dev)
        n_new = torch.zeros(U, **i32)
        trellis = torch.zeros(S, trellis_words(U, beam), **i32)
        d = DecDims(R, Tp, E, A, C, NL, V, 1, int(loc), ops._prec)
        St = dict(tok=tok, xin=torch.zeros(1, R, C + E, **f32), q=torch.zeros(1, R, A, **f32), att=attb, hs=hs, cs=cs,
                  gates=torch.zeros(NL, 1, R, 4 * C, **f32), ebuf=torch.zeros(R, Tp, **f32), logits_step=torch.zeros(R, V, **f32))
        if loc:
            St['f'] = torch.zeros(1, R, LOC_C, Tp, **f32)
            St['s'] = torch.zeros(1, R, Tp, A, dtype=s_dtype(d.prec), device=dev)
        st = DecState()
        for k, v in St.items():
            setattr(st, k, v.data_ptr())
        logits = torch.zeros(R, V, **f32)
        cur = torch.zeros(R, V, **f32)
        topv = torch.zeros(R, kb, **f32)
        topi = torch.zeros(R, kb, **i32)
        stream = cur_stream()
        d_, p_, st_ = ctypes.byref(d), ctypes.byref(params), ctypes.byref(st)
        # ---- the loop: enqueue only (no read-back, no allocation, no host-built tensor)
        for t in range(S):
            check(L_.las_decoder_step(d_, p_, ptr(encB), ptr(psiB), ptr(lenB), st_, ptr(logits), stream), 'las_decoder_step')
            check(L_.las_log_softmax_rows(ptr(logits), I(R), I(V), ptr(cur), stream), 'las_log_softmax_rows')
            if joint_ctc:
                check(L_.las_topk_rows(ptr(cur), I(R), I(V), I(K), ptr(cv), ptr(cand), stream), 'las_topk_rows')
                check(L_.las_ctc_prefix_score_batch(ptr(lp), I(U), I(Tp), I(V), ptr(enc_len_dev), ptr(row_utt), ptr(r_prev), ptr(tok),
                                                    ptr(plen), ptr(cand), I(R), I(K), ptr(psi_c), ptr(r_out), stream),
                      'las_ctc_prefix_score_batch')
                check(L_.las_beam_combine(ptr(cur), I(R), I(V), ptr(cand), ptr(psi_c), ptr(prev_ctc), I(K), F(lam), stream),
                      'las_beam_combine')
            check(L_.las_topk_rows(ptr(cur), I(R), I(V), I(kb), ptr(topv), ptr(topi), stream), 'las_topk_rows')
            check(L_.las_beam_select(ptr(topv), ptr(topi), ptr(cand), I(U), I(beam), I(kb), I(K), ptr(n_live), ptr(ssum), ptr(plen),
                                     ptr(limit), I(t), ptr(parent), ptr(tok_n), ptr(j_n), ptr(plen_n), ptr(sum_n), ptr(n_new),
                                     P(trellis.data_ptr() + 4 * t * trellis_words(U, beam)), stream), 'las_beam_select')
            check(L_.las_beam_gather(I(U), I(beam), I(NL), I(C), I(Tp), I(K), ptr(enc_len_dev), ptr(limit), I(t), ptr(n_new), ptr(parent),
                                     ptr(j_n), ptr(tok_n), ptr(plen_n), ptr(sum_n), ptr(hs), ptr(cs), ptr(attb) if loc else None,
                                     ptr(r_out), ptr(psi_c), ptr(r_prev), ptr(prev_ctc), ptr(tok), ptr(plen), ptr(ssum), ptr(n_live),
                                     stream), 'las_beam_gather')
        host = trellis.cpu().numpy()                                    # the one D2H copy (synchronises)
    return rebuild_hypotheses(host, U, beam, steps)
