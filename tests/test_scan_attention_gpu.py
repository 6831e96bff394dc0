"""GPU: SCAN attention maps, per-word / per-region similarities and scores of listed pairs (ops.scan_pair_attention,
ops.scan_candidate_attention, csrc/scan_attn.hip) against oracle/itr_oracle.py: O.func_attention returns the attention matrix
(Objectives.py:421-476), O.xattn_score the score; the per-item cosine is restated here from Objectives.py:10-15.
Bound: the project's 2e-5 (test_edges_gpu.py, golden G5), absolute; relative to max(1, |oracle|) for the scores of agg_func='Sum'.
Every pair of every case is compared: the number of compared elements is asserted equal to the number produced."""
import numpy as np
import pytest
import torch

import itr_oracle as O
from itr_amd import ops

pytestmark = pytest.mark.gpu

NORMS = ['clipped_l2norm', 'l2norm', 'softmax', 'no_norm', 'clipped', 'l1norm', 'clipped_l1norm']
AGGS = ['LogSumExp', 'Mean', 'Max', 'Sum']
TOL = 2e-5
NI = 9
LENS = [1, 15, 16, 17, 48, 64, 65, 96, 7, 12, 33, 82, 5, 20]          # 14 captions
R = 36


def make_set(seed, D, lens=LENS, Ni=NI):
    torch.manual_seed(seed)
    lens = np.asarray(lens, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    img = O.l2norm(torch.randn(Ni, R, D), -1)
    words = torch.randn(int(lens.sum()), D) * 0.5
    cap = torch.zeros(len(lens), int(lens.max()), D)
    for c, (o, l) in enumerate(zip(off, lens)):
        cap[c, :l] = words[o:o + l]
    return img, words, cap, off, lens


def cosine(x1, x2, eps=1e-8):
    """cosine_similarity, Objectives.py:10-15: w12 / (w1 * w2).clamp(min=eps) along the last dim"""
    w12 = torch.sum(x1 * x2, -1)
    w1 = torch.norm(x1, 2, -1)
    w2 = torch.norm(x2, 2, -1)
    return w12 / (w1 * w2).clamp(min=eps)


def oracle_pairs(img, cap, lens, xa, norm, agg, lambda_softmax=9.0):
    """-> attn[c] (Ni, W, R) word-major, row_sim[c] (Ni, W | R), S (Ni, Nc), from the oracle as it is"""
    attn, sims = [], []
    for c in range(cap.shape[0]):
        w = int(lens[c])
        e = cap[c, :w].unsqueeze(0).expand(img.shape[0], w, -1)
        if xa == 't2i':
            ctx, a = O.func_attention(e, img, norm, lambda_softmax)          # a (Ni, W, R)
            sims.append(cosine(e, ctx))
        else:
            ctx, a = O.func_attention(img, e, norm, lambda_softmax)          # a (Ni, R, W)
            a = a.transpose(1, 2)
            sims.append(cosine(img, ctx))
        attn.append(a.contiguous())
    return attn, sims, O.xattn_score(img, cap, lens, xa, norm, agg)


def all_pairs(Ni, Nc, rng=None):
    pairs = np.stack(np.meshgrid(np.arange(Ni), np.arange(Nc), indexing='ij'), -1).reshape(-1, 2).astype(np.int32)
    if rng is not None:
        pairs = pairs[rng.permutation(len(pairs))]
    return pairs


def agg64(sim, agg, lambda_lse=6.0):
    sim = np.asarray(sim, np.float64)
    if agg == 'LogSumExp':
        return np.log(np.exp(sim * lambda_lse).sum()) / lambda_lse
    return {'Max': sim.max, 'Sum': sim.sum, 'Mean': sim.mean}[agg]()


@pytest.mark.parametrize("xa", ['t2i', 'i2t'])
@pytest.mark.parametrize("D", [64, 1024])
def test_oracle_parity_and_structure(dev, D, xa):
    img, words, cap, off, lens = make_set(3 + D, D)
    Nc = len(lens)
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d = img.to(dev), words.to(dev)
    ws = ops.scan_pairs_prepare(img_d, words_d, plan, xa)
    rng = np.random.RandomState(D)
    worst = {'attn': 0.0, 'row_sim': 0.0, 'score': 0.0, 'sum1': 0.0, 'agg': 0.0, 'vs_scores': 0.0}
    bit_equal = True
    for norm in NORMS:
        for agg in AGGS:
            o_attn, o_sim, o_S = oracle_pairs(img, cap, lens, xa, norm, agg)
            pairs = all_pairs(NI, Nc, rng)
            got = ops.scan_pair_attention(img_d, words_d, plan, torch.from_numpy(pairs).to(dev), cross_attn=xa, raw_feature_norm=norm,
                                          agg_func=agg, workspace=ws)
            P = len(pairs)
            assert len(got) == P and got.attn_ptr.shape == (P + 1,) and got.row_ptr.shape == (P + 1,)
            assert np.array_equal(got.cap_len.cpu().numpy(), lens[pairs[:, 1]])
            assert np.array_equal(got.row_ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(lens[pairs[:, 1]].astype(np.int64))]))
            assert np.array_equal(got.attn_ptr.cpu().numpy(), got.row_ptr.cpu().numpy() * R)
            n_attn = n_sim = n_score = 0
            score = got.score.cpu().numpy()
            e_attn = e_sim = e_score = e_sum1 = e_agg = 0.0
            for p, (i, c) in enumerate(pairs):
                A = got.matrix(p).cpu()
                assert A.shape == (lens[c], R)
                sim = got.sims(p).cpu()
                assert sim.shape == ((lens[c],) if xa == 't2i' else (R,))
                e_attn = max(e_attn, float((A - o_attn[c][i]).abs().max()))
                e_sim = max(e_sim, float((sim - o_sim[c][i]).abs().max()))
                want = float(o_S[i, c])
                scale = max(1.0, abs(want)) if agg == 'Sum' else 1.0
                e_score = max(e_score, abs(float(score[p]) - want) / scale)
                e_sum1 = max(e_sum1, float((A.double().sum(1 if xa == 't2i' else 0) - 1.0).abs().max()))
                e_agg = max(e_agg, abs(agg64(sim.numpy(), agg) - float(score[p])) / scale)
                n_attn += A.numel()
                n_sim += sim.numel()
                n_score += 1
            assert n_attn == got.attn.numel() == int(lens[pairs[:, 1]].sum()) * R
            assert n_sim == got.row_sim.numel() and n_score == got.score.numel() == NI * Nc
            # the score-only path on the same pairs
            cand = torch.arange(NI, device=dev, dtype=torch.int32).repeat(Nc, 1)
            sc = ops.scan_candidate_scores(img_d, words_d, plan, cand, 'caption', cross_attn=xa, raw_feature_norm=norm, agg_func=agg).cpu().numpy()
            e_vs = float(np.abs(sc[pairs[:, 1], pairs[:, 0]].astype(np.float64) - score).max())
            short = lens[pairs[:, 1]] <= 64
            eq = np.array_equal(sc[pairs[:, 1], pairs[:, 0]][short].view(np.uint32), score[short].view(np.uint32))
            bit_equal = bit_equal and eq
            print("D=%d %s %s %s: attn %.3g row_sim %.3g score %.3g | sums-1 %.3g host-agg %.3g vs scores %.3g (<= 64 words bit-equal: %s)"
                  % (D, xa, norm, agg, e_attn, e_sim, e_score, e_sum1, e_agg, e_vs, eq))
            for key, v in (('attn', e_attn), ('row_sim', e_sim), ('score', e_score), ('sum1', e_sum1), ('agg', e_agg), ('vs_scores', e_vs)):
                worst[key] = max(worst[key], v)
            assert e_attn <= TOL and e_sim <= TOL and e_score <= TOL, (D, xa, norm, agg, e_attn, e_sim, e_score)
            assert e_sum1 <= 1e-5, (D, xa, norm, agg, e_sum1)
            assert e_agg <= TOL, (D, xa, norm, agg, e_agg)
            assert e_vs <= TOL, (D, xa, norm, agg, e_vs)
    print("worst D=%d %s: %s; scores of captions <= 64 words bit-equal to scan_candidate_scores: %s" % (D, xa, worst, bit_equal))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("xa", ['t2i', 'i2t'])
def test_a_pairs_outputs_are_its_own(dev, xa):
    """alone, listed twice, and among all others in shuffled order: identical bits in attn, row_sim and score; and through both
    directions of the list form"""
    D = 256
    img, words, cap, off, lens = make_set(17, D)
    Nc = len(lens)
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d = img.to(dev), words.to(dev)
    rng = np.random.RandomState(5)
    for norm, agg in (('clipped_l2norm', 'LogSumExp'), ('softmax', 'Mean'), ('l1norm', 'Max'), ('no_norm', 'Sum')):
        kw = dict(cross_attn=xa, raw_feature_norm=norm, agg_func=agg)
        pairs = all_pairs(NI, Nc, rng)
        full = ops.scan_pair_attention(img_d, words_d, plan, torch.from_numpy(pairs).to(dev), **kw)
        n_checked = 0
        for p in range(0, len(pairs), 5):
            one = torch.from_numpy(pairs[p:p + 1]).to(dev)
            alone = ops.scan_pair_attention(img_d, words_d, plan, one, **kw)
            twice = ops.scan_pair_attention(img_d, words_d, plan, torch.cat([one, one]), **kw)
            for other, q in ((alone, 0), (twice, 0), (twice, 1)):
                assert torch.equal(bits(other.matrix(q)), bits(full.matrix(p))), (norm, agg, p)
                assert torch.equal(bits(other.sims(q)), bits(full.sims(p))), (norm, agg, p)
                assert torch.equal(bits(other.score[q]), bits(full.score[p])), (norm, agg, p)
                n_checked += 1
        assert n_checked == 3 * len(range(0, len(pairs), 5))
        # list form: by caption (every image for every caption) and by image (every caption for every image) hold the same pairs
        m = 4
        cand_c = torch.from_numpy(np.stack([rng.permutation(NI) for _ in range(Nc)]).astype(np.int32)).to(dev)
        cand_i = torch.from_numpy(np.stack([rng.permutation(Nc) for _ in range(NI)]).astype(np.int32)).to(dev)
        by_c = ops.scan_candidate_attention(img_d, words_d, plan, cand_c, 'caption', **kw)          # m=None: all columns
        by_i = ops.scan_candidate_attention(img_d, words_d, plan, cand_i, 'image', **kw)
        assert len(by_c) == len(by_i) == NI * Nc
        where = {(int(i), int(c)): q for q, (i, c) in enumerate(by_i.pairs.cpu().numpy())}
        for q, (i, c) in enumerate(by_c.pairs.cpu().numpy()):
            assert (i, c) == (int(cand_c[c, q % NI]), q // NI)
            o = where[(int(i), int(c))]
            assert torch.equal(bits(by_c.matrix(q)), bits(by_i.matrix(o)))
            assert torch.equal(bits(by_c.sims(q)), bits(by_i.sims(o)))
            assert torch.equal(bits(by_c.score[q]), bits(by_i.score[o]))
        first = ops.scan_candidate_attention(img_d, words_d, plan, cand_c, 'caption', m=m, **kw)
        assert len(first) == Nc * m
        for c in range(Nc):
            for k in range(m):
                assert tuple(first.pairs[c * m + k].tolist()) == (int(cand_c[c, k]), c)
                assert torch.equal(bits(first.matrix(c * m + k)), bits(by_c.matrix(c * NI + k)))


@pytest.mark.parametrize("xa", ['t2i', 'i2t'])
def test_refusals_and_empty(dev, xa):
    D = 64
    img, words, cap, off, lens = make_set(5, D)
    Nc = len(lens)
    plan = ops.ScanPlan(off, lens, words.shape[0], dev)
    img_d, words_d = img.to(dev), words.to(dev)
    pairs = torch.zeros(3, 2, dtype=torch.int32, device=dev)
    # 97 words
    p97 = ops.ScanPlan(np.asarray([0, 5], np.int64), np.asarray([5, 97], np.int32), 102, dev)
    with pytest.raises(NotImplementedError):
        ops.scan_pair_attention(img_d, torch.zeros(102, D, device=dev), p97, pairs, cross_attn=xa)
    # 35 regions
    with pytest.raises(NotImplementedError):
        ops.scan_pair_attention(torch.zeros(NI, 35, D, device=dev), words_d, plan, pairs, cross_attn=xa)
    # an index out of range, either column, either side
    for col, bad in ((0, -1), (0, NI), (1, -1), (1, Nc)):
        q = pairs.clone()
        q[1, col] = bad
        with pytest.raises(ValueError):
            ops.scan_pair_attention(img_d, words_d, plan, q, cross_attn=xa)
    cand = torch.zeros(Nc, 3, dtype=torch.int32, device=dev)
    cand[2, 1] = NI
    with pytest.raises(ValueError):
        ops.scan_candidate_attention(img_d, words_d, plan, cand, 'caption', cross_attn=xa)
    # a workspace prepared for the other direction, and something that is no workspace
    other = ops.scan_pairs_prepare(img_d, words_d, plan, 'i2t' if xa == 't2i' else 't2i')
    with pytest.raises(ValueError):
        ops.scan_pair_attention(img_d, words_d, plan, pairs, cross_attn=xa, workspace=other)
    with pytest.raises(TypeError):
        ops.scan_pair_attention(img_d, words_d, plan, pairs, cross_attn=xa, workspace=other.buf)
    with pytest.raises(ValueError):
        ops.scan_pair_attention(img_d, words_d, plan, pairs, cross_attn=xa, raw_feature_norm='bogus')
    with pytest.raises(ValueError):
        ops.scan_pair_attention(img_d, words_d, plan, pairs, cross_attn=xa, agg_func='bogus')
    with pytest.raises(ValueError):
        ops.scan_pair_attention(img_d, words_d, plan, pairs, cross_attn='bogus')
    with pytest.raises(ValueError):
        ops.scan_candidate_attention(img_d, words_d, plan, cand, 'bogus', cross_attn=xa)
    with pytest.raises(ValueError):
        ops.scan_pair_attention(img_d, words_d, plan, pairs[:, :1], cross_attn=xa)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scan_pair_attention(img, words_d, plan, pairs, cross_attn=xa)
    # P = 0
    e = ops.scan_pair_attention(img_d, words_d, plan, pairs[:0], cross_attn=xa)
    assert len(e) == 0 and e.attn.shape == (0,) and e.row_sim.shape == (0,) and e.score.shape == (0,) and e.cap_len.shape == (0,)
    assert e.attn_ptr.tolist() == [0] and e.row_ptr.tolist() == [0]
    e = ops.scan_candidate_attention(img_d, words_d, plan, cand, 'caption', m=0, cross_attn=xa)
    assert len(e) == 0
    # the device is alive and the results right after every refusal
    torch.cuda.synchronize()
    ok = ops.scan_pair_attention(img_d, words_d, plan, pairs, cross_attn=xa)
    a, _, S = oracle_pairs(img, cap, lens, xa, 'clipped_l2norm', 'LogSumExp')
    assert float((ok.matrix(0).cpu() - a[0][0]).abs().max()) <= TOL and abs(float(ok.score[0]) - float(S[0, 0])) <= TOL
