"""GPU: ops.rank_positions / rank_gather_keys (csrc/rank_gt.hip) -- the position of every positive of a general ground-truth
relation in its query's ranked list -- against a stable numpy argsort.  Every comparison of positions is exact integer equality.
Shapes sit at the kernels' seams: one element, columns below and across a lane's 4 columns, a 256-column strip and a 1 024-column
tile, rows across 64 and 128; relations from no positive to the whole gallery and just above what one pass holds in LDS
(256 thresholds of a row, 2 048 of a 256-column strip)."""
import numpy as np
import pytest
import torch

from itr_amd import ops
from itr_amd.metricmodule import evaluation

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 37), (3, 4), (65, 33), (130, 1027), (300, 2100)]
VALUES = ['continuous', 'ties', 'equal', 'special']
ROW_CAP, STRIP, COL_CAP = 256, 256, 2048          # GT_ROW_CAP, GT_STRIP, GT_COL_CAP of csrc/rank_gt.hip


# ---- the CPU reference ------------------------------------------------------------------------------------------------------
def canon(a):
    return np.where(np.isnan(a), np.inf, a) + 0.0          # NaN as +inf, -0.0 -> +0.0


def positions(line, idx):
    order = np.argsort(canon(line), kind='stable')[::-1]   # larger first, the higher index on a tie
    where = np.empty(len(line), dtype=np.int64)
    where[order] = np.arange(len(line))
    return where[idx]


def ref_positions(S, gt_host):
    ip, ic, cp, ci = gt_host
    i2t = [positions(S[i], ic[ip[i]:ip[i + 1]]) for i in range(len(ip) - 1)]
    t2i = [positions(S[:, j], ci[cp[j]:cp[j + 1]]) for j in range(len(cp) - 1)]
    z = [np.zeros(0, dtype=np.int64)]
    return np.concatenate(i2t + z), np.concatenate(t2i + z)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def scores(kind, Ni, Nc, seed, dtype=np.float32):
    rng = np.random.RandomState(seed)
    if kind == 'continuous':
        return rng.randn(Ni, Nc).astype(dtype)
    if kind == 'ties':
        return rng.randint(0, 4, size=(Ni, Nc)).astype(dtype)
    if kind == 'equal':
        return np.full((Ni, Nc), 0.25, dtype=dtype)
    S = rng.randint(-1, 2, size=(Ni, Nc)).astype(dtype)    # -1, 0, 1 with signed zeros, infinities and NaN sprinkled in
    S[S == 0] = np.where(rng.rand(int((S == 0).sum())) < 0.5, -0.0, 0.0)
    pick = rng.rand(Ni, Nc)
    S[pick < 0.08] = np.nan
    S[(pick >= 0.08) & (pick < 0.14)] = np.inf
    S[(pick >= 0.14) & (pick < 0.20)] = -np.inf
    return S


def relation_pairs(kind, Ni, Nc, seed):
    """(image, caption) pairs.  'random': 0 .. 40 positives per image, image 1 and the middle caption without any, a positive in the
    first and in the last column.  'layout': caption j <-> image j // 5.  'dense': random + what is just above one pass of the
    kernels (an image with ROW_CAP + 1 positives, a strip of columns with more than COL_CAP in all) or, on small matrices, a row
    and a column whose positives are the whole gallery."""
    rng = np.random.RandomState(seed)
    if kind == 'layout':
        cap = np.arange(Nc)
        return np.stack([cap // 5, cap], 1)[cap // 5 < Ni]
    rel = np.zeros((Ni, Nc), dtype=bool)
    for i in range(Ni):
        rel[i, rng.choice(Nc, size=min(Nc, rng.randint(0, 41)), replace=False)] = True
    if Ni > 1:
        rel[1, :] = False                                    # an image without positives
    if Nc > 2:
        rel[:, Nc // 2] = False                              # a caption without positives
    rel[0, 0] = rel[0, Nc - 1] = True
    if kind == 'dense':
        if Nc > ROW_CAP + 1:
            rel[min(7, Ni - 1), rng.choice(Nc, size=ROW_CAP + 1, replace=False)] = True
        else:
            rel[min(2, Ni - 1), :] = True
        if Ni * STRIP > COL_CAP + STRIP and Nc >= 2 * STRIP:
            per = COL_CAP // STRIP + 1                       # 9 positives in each of the 256 columns of the second strip
            for j in range(STRIP, 2 * STRIP):
                rel[rng.choice(Ni, size=per, replace=False), j] = True
        else:
            rel[:, min(5, Nc - 1)] = True
    pairs = np.argwhere(rel)
    return pairs[rng.permutation(len(pairs))]                # (the order of the pairs must not matter)


def layouts_of(S, dev):
    """The same matrix contiguous, as a view with an odd row stride, and as a view starting one float past a 16-byte boundary."""
    Ni, Nc = S.shape
    t = torch.from_numpy(S)
    out = [t.to(dev)]
    ld = Nc + 1 if Nc % 2 == 0 else Nc + 2
    buf = torch.full((Ni, ld), float('nan'), dtype=t.dtype, device=dev)
    buf[:, :Nc] = t.to(dev)
    out.append(buf[:, :Nc])
    ld4 = (Nc + 3) // 4 * 4
    flat = torch.full((Ni * ld4 + 1,), float('nan'), dtype=t.dtype, device=dev)
    view = flat[1:].view(Ni, ld4)[:, :Nc]
    view.copy_(t.to(dev))
    assert view.data_ptr() % 16 == t.element_size() % 16
    out.append(view)
    return out


_cache = {}


def case(kind_v, kind_r, Ni, Nc, dtype=np.float32):
    """(S, pairs, host CSR, reference positions): computed once, shared, never modified."""
    key = (kind_v, kind_r, Ni, Nc, np.dtype(dtype).name)
    if key not in _cache:
        S = scores(kind_v, Ni, Nc, seed=Ni * 7 + Nc, dtype=dtype)
        pairs = relation_pairs(kind_r, Ni, Nc, seed=Ni + Nc)
        host = ops.ground_truth_csr(pairs, Ni, Nc)
        _cache[key] = (S, pairs, host, ref_positions(S, host))
    return _cache[key]


def check(got, want, what):
    i_pos, t_pos = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert i_pos.dtype == np.int32 and t_pos.dtype == np.int32
    assert np.array_equal(i_pos, want[0]), (what, 'i2t', int((i_pos != want[0]).sum()), len(i_pos))
    assert np.array_equal(t_pos, want[1]), (what, 't2i', int((t_pos != want[1]).sum()), len(t_pos))


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind_v", VALUES)
@pytest.mark.parametrize("Ni,Nc", SHAPES)
def test_positions_equal_the_stable_argsort(dev, Ni, Nc, kind_v):
    for kind_r in ('random', 'layout', 'dense'):
        S, pairs, host, want = case(kind_v, kind_r, Ni, Nc)
        gt = ops.GroundTruth(pairs, Ni, Nc, dev)
        assert gt.nnz == len(pairs) and np.array_equal(gt.img_ptr_host, host[0]) and np.array_equal(gt.cap_ptr.cpu().numpy(), host[2])
        for n_layout, S_dev in enumerate(layouts_of(S, dev)):
            check(ops.rank_positions(S_dev, gt), want, (Ni, Nc, kind_v, kind_r, n_layout))


def test_dense_relations_hold_what_they_promise():
    """The 'dense' relation does cross one pass of each kernel on the large shapes, and holds a whole-gallery row and column on
    65 x 33, whose positions are a permutation."""
    for Ni, Nc in ((130, 1027), (300, 2100)):
        ip, ic, cp, ci = case('ties', 'dense', Ni, Nc)[2]
        assert np.diff(ip).max() > ROW_CAP
    cp = case('ties', 'dense', 300, 2100)[2][2]
    assert cp[2 * STRIP] - cp[STRIP] > COL_CAP
    S, pairs, (ip, ic, cp, ci), (i_pos, t_pos) = case('ties', 'dense', 65, 33)
    assert ip[3] - ip[2] == 33 and sorted(i_pos[ip[2]:ip[3]].tolist()) == list(range(33))
    assert cp[6] - cp[5] == 65 and sorted(t_pos[cp[5]:cp[6]].tolist()) == list(range(65))


def test_whole_gallery_queries_return_a_permutation(dev):
    S, pairs, (ip, ic, cp, ci), want = case('ties', 'dense', 65, 33)
    full = np.stack(np.meshgrid(np.arange(65), np.arange(33), indexing='ij'), -1).reshape(-1, 2)          # every pair a positive
    gt = ops.GroundTruth(full, 65, 33, dev)
    i_pos, t_pos, _ = ops.rank_positions(torch.from_numpy(S).to(dev), gt)
    i_pos, t_pos = i_pos.cpu().numpy().reshape(65, 33), t_pos.cpu().numpy().reshape(33, 65)
    assert (np.sort(i_pos, 1) == np.arange(33)).all() and (np.sort(t_pos, 1) == np.arange(65)).all()
    check((torch.from_numpy(i_pos.ravel()), torch.from_numpy(t_pos.ravel())), ref_positions(S, ops.ground_truth_csr(full, 65, 33)), 'full')


@pytest.mark.parametrize("im_div", [5, 1, 3])
def test_layout_relation_gives_the_rankers_vectors(dev, im_div):
    Ni = 130
    Nc = Ni * im_div
    for kind_v in ('continuous', 'ties', 'special'):
        S = torch.from_numpy(scores(kind_v, Ni, Nc, seed=im_div)).to(dev)
        gt = ops.GroundTruth.from_layout(Ni, Nc, im_div, dev)
        i_pos, t_pos, _ = ops.rank_positions(S, gt)
        i_rank, _, t_rank, _, _ = ops.rank_counts(S, im_div)
        assert gt.nnz == Nc and torch.equal(i_pos.view(Ni, im_div).min(1).values, i_rank)
        assert torch.equal(t_pos, t_rank)


@pytest.mark.parametrize("kind_v", ['continuous', 'ties'])
def test_row_blocks_in_any_order_equal_the_whole_matrix(dev, kind_v):
    Ni, Nc = 300, 2100
    S, pairs, host, want = case(kind_v, 'dense', Ni, Nc)
    gt = ops.GroundTruth(pairs, Ni, Nc, dev)
    S_dev = torch.from_numpy(S).to(dev)
    whole = ops.rank_positions(S_dev, gt)
    check(whole, want, 'whole')
    for block in (64, 100, 299):
        cuts = [(r, min(r + block, Ni)) for r in range(0, Ni, block)]
        for order in (cuts, cuts[::-1]):
            state = None
            for a, b in order:
                state = ops.rank_gather_keys(S_dev[a:b], gt, a, state)
            for a, b in order:
                i_pos, t_pos, state2 = ops.rank_positions(S_dev[a:b], gt, a, state)
                assert state2 is state
            assert torch.equal(i_pos, whole[0]) and torch.equal(t_pos, whole[1]), (block, order[0])


@pytest.mark.parametrize("Ni,Nc", [(65, 33), (130, 1027)])
def test_float64_matrices_are_ranked_in_float64(dev, Ni, Nc):
    rng = np.random.RandomState(Ni)
    base = scores('ties', Ni, Nc, seed=3).astype(np.float64)
    S = base + rng.randint(-2, 3, size=base.shape) * 2.0 ** -40          # differences far below an fp32 ulp of 1.0 (2^-23); exact ties stay
    S[rng.rand(Ni, Nc) < 0.05] = np.nan
    S[rng.rand(Ni, Nc) < 0.05] = -0.0
    assert (S.astype(np.float32).astype(np.float64) != S)[~np.isnan(S)].any()
    for kind_r in ('random', 'dense'):
        pairs = relation_pairs(kind_r, Ni, Nc, seed=Ni + Nc)
        host = ops.ground_truth_csr(pairs, Ni, Nc)
        gt = ops.GroundTruth(pairs, Ni, Nc, dev)
        want = ref_positions(S, host)
        for S_dev in layouts_of(S, dev):
            check(ops.rank_positions(S_dev, gt), want, (Ni, Nc, kind_r, 'f64'))
        as32 = ref_positions(S.astype(np.float32), host)
        assert not np.array_equal(as32[0], want[0])                       # fp32 would have merged scores that float64 separates


def test_refusals(dev):
    with pytest.raises(ValueError, match="out of range"):
        ops.GroundTruth([[0, 0], [3, 1]], 3, 4, dev)
    with pytest.raises(ValueError, match="more than once"):
        ops.GroundTruth([[0, 1], [2, 3], [0, 1]], 3, 4, dev)
    gt = ops.GroundTruth([[0, 1], [2, 3]], 3, 4, dev)
    S = torch.zeros(3, 4, device=dev)
    with pytest.raises(ValueError, match="relation is over"):
        ops.rank_positions(torch.zeros(3, 5, device=dev), gt)             # gallery size mismatch: captions
    with pytest.raises(ValueError, match="relation is over"):
        ops.rank_positions(torch.zeros(4, 4, device=dev), gt)             # ... images
    with pytest.raises(ValueError, match="whole matrix"):
        ops.rank_positions(S[:2], gt)                                     # a row block without a state
    with pytest.raises(ValueError, match="float64"):
        ops.rank_gather_keys(S[:2].double(), gt, 0)                       # a float64 row block
    with pytest.raises(ValueError, match="float64"):
        ops.rank_positions(S.double(), gt, 0, ops.rank_gather_keys(S, gt))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rank_positions(S.cpu(), gt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rank_gather_keys(S.cpu(), gt)
    with pytest.raises(TypeError):
        ops.rank_positions(S.half(), gt)
    # an empty relation, an empty gallery
    i_pos, t_pos, _ = ops.rank_positions(S, ops.GroundTruth(np.zeros((0, 2), dtype=np.int64), 3, 4, dev))
    assert i_pos.numel() == 0 and t_pos.numel() == 0 and i_pos.dtype == torch.int32
    i_pos, t_pos, _ = ops.rank_positions(torch.zeros(0, 4, device=dev), ops.GroundTruth(np.zeros((0, 2), dtype=np.int64), 0, 4, dev))
    assert i_pos.numel() == 0 and t_pos.numel() == 0


def brute_metrics(S, host, direction, ks=(1, 5, 10)):
    """The definitions from the SORTED LISTS, query by query, in float64."""
    ip, ic, cp, ci = host
    ptr, idx, lines = (ip, ic, S) if direction == 'i2t' else (cp, ci, S.T)
    best, rp, ap, none = [], [], [], 0
    for q in range(len(ptr) - 1):
        pos_set = set(idx[ptr[q]:ptr[q + 1]].tolist())
        if not pos_set:
            none += 1
            continue
        ranked = np.argsort(canon(lines[q]), kind='stable')[::-1]
        R = len(pos_set)
        hits = [k for k, item in enumerate(ranked.tolist()) if item in pos_set]
        best.append(hits[0])
        rp.append(sum(1 for k in hits if k < R) / R)
        ap.append(sum((j + 1) / (k + 1) for j, k in enumerate(hits) if k < R) / R)
    n = len(best)
    out = {'r@%d' % k: 100.0 * sum(1 for b in best if b < k) / n for k in ks}
    out.update(medr=float(np.floor(np.median(best)) + 1), meanr=float(np.mean(best)) + 1, rprecision=100.0 * float(np.mean(rp)),
               map_at_r=100.0 * float(np.mean(ap)), n_queries=n, n_without_positives=none)
    return out


def test_gt_metrics(dev):
    Ni, Nc = 130, 1027
    S, pairs, host, want = case('continuous', 'random', Ni, Nc)
    res = evaluation.gt_metrics(S, ops.GroundTruth(pairs, Ni, Nc, dev))
    for d, w in (('i2t', want[0]), ('t2i', want[1])):
        assert np.array_equal(res[d]['positions'], w)
        for k, v in brute_metrics(S, host, d).items():
            assert abs(res[d][k] - v) <= 1e-12, (d, k, res[d][k], v)
    assert res['i2t']['n_without_positives'] >= 1 and res['t2i']['n_without_positives'] >= 1
    # the layout relation: the reference's five numbers, to the last bit (fp32 and float64 matrices)
    Nc = Ni * 5
    for dtype in (np.float32, np.float64):
        S = scores('continuous', Ni, Nc, seed=11, dtype=dtype)
        res = evaluation.gt_metrics(S, ops.GroundTruth.from_layout(Ni, Nc, 5, dev))
        ref = evaluation.cal_recall(S)
        for d in ('i2t', 't2i'):
            for k, name in (('r@1', 'r1'), ('r@5', 'r5'), ('r@10', 'r10'), ('medr', 'medr'), ('meanr', 'meanr')):
                assert res[d][k] == ref['%s_%s' % (d, name)], (d, k)
            assert np.array_equal(res[d]['best'], ref['%s_ranks' % d])
