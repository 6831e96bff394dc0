"""oracle/itr_oracle.py's sgraf_similarity restated WITH its intermediates: the oracle returns scores only, the explaining entry
points (ops.sgraf_pair_attention) also return SCAN_attention's softmax weights, AttentionFiltration's node weights and
GraphReasoning's edges.  Statement for statement the oracle's code, built from its own pieces (O._linear, O._bn_eval, O.l2norm,
O.l1norm, O._LEAKY, O.sgraf_visual_sa / sgraf_text_sa), so that on the CPU the scores are BIT-EQUAL to O.sgraf_similarity --
which every user of this module asserts first (`assert_restates_oracle`)."""
import torch
import torch.nn.functional as F

import itr_oracle as O


def sgraf_similarity_explained(w, img_emb, cap_emb, cap_lens, module_name='SAF', sgr_step=3):
    """-> (S [Ni, Nc], per caption c a dict: 'attn' [Ni, W, 36], and 'node_w' [Ni, W + 1] (SAF) or 'edge' [sgr_step, Ni, W + 1, W + 1]
    (SGR); node 0 is the global node)"""
    n_image = img_emb.shape[0]
    img_glo = O.sgraf_visual_sa(w, img_emb, img_emb.mean(1))
    cols, parts = [], []
    for c in range(cap_emb.shape[0]):
        nw = int(cap_lens[c])
        cap_i = cap_emb[c, :nw].unsqueeze(0)
        cap_exp = cap_i.expand(n_image, nw, -1)
        cap_glo = O.sgraf_text_sa(w, cap_i, cap_i.mean(1))
        # sgraf_scan_attention(cap_exp, img_emb, smooth=9.0), keeping the softmax
        attn = torch.bmm(img_emb, cap_exp.transpose(1, 2))
        attn = O.l2norm(F.leaky_relu(attn, O._LEAKY), 2)
        attn = torch.softmax(attn.transpose(1, 2) * 9.0, dim=2)
        ctx = O.l2norm(torch.bmm(attn, img_emb), dim=-1)
        part = {'attn': attn}
        sim_loc = O.l2norm(O._linear((ctx - cap_exp).pow(2), w, 'sim_tranloc_w'), dim=-1)
        sim_glo = O.l2norm(O._linear((img_glo - cap_glo).pow(2), w, 'sim_tranglo_w'), dim=-1)
        sim_emb = torch.cat([sim_glo.unsqueeze(1), sim_loc], 1)
        if module_name == 'SGR':
            edges = []
            for k in range(sgr_step):
                p = 'SGR_module.sgr%d' % k
                q = O._linear(sim_emb, w, p + '.graph_query_w')
                kk = O._linear(sim_emb, w, p + '.graph_key_w')
                edge = torch.softmax(torch.bmm(q, kk.transpose(1, 2)), dim=-1)
                edges.append(edge)
                sim_emb = torch.relu(O._linear(torch.bmm(edge, sim_emb), w, p + '.sim_graph_w'))
            sim_vec = sim_emb[:, 0]
            part['edge'] = torch.stack(edges, 0)
        elif module_name == 'SAF':
            a = O._linear(sim_emb, w, 'SAF_module.attn_sim_w').transpose(1, 2)
            a = O.l1norm(torch.sigmoid(O._bn_eval(a, w, 'SAF_module.bn', 1)), dim=-1)
            part['node_w'] = a.squeeze(1)
            sim_vec = O.l2norm(torch.bmm(a, sim_emb).squeeze(1), dim=-1)
        else:
            raise ValueError('Invalid input of config.module_name in configs.py')
        cols.append(torch.sigmoid(O._linear(sim_vec, w, 'sim_eval_w')).squeeze(1))
        parts.append(part)
    return torch.stack(cols, 1), parts


def assert_restates_oracle(S, w, img_emb, cap_emb, cap_lens, module_name, sgr_step=3):
    want = O.sgraf_similarity(w, img_emb, cap_emb, cap_lens, module_name, sgr_step)
    assert torch.equal(S, want), "the restatement's scores are not bit-equal to O.sgraf_similarity"


def to_double(w, *tensors):
    return ({k: v.double() for k, v in w.items()},) + tuple(t.double() for t in tensors)


def flat_blocks(parts, pairs, key):
    """the blocks of `key` for pairs [(image, caption)] concatenated as the flat output buffers lay them out -> 1-D float64 numpy"""
    import numpy as np
    out = []
    for i, c in pairs:
        t = parts[int(c)][key]
        t = t[:, int(i)] if key == 'edge' else t[int(i)]
        out.append(t.reshape(-1).double().numpy())
    return np.concatenate(out) if out else np.zeros(0)
