"""The toy precomp dataset and tiny checkpoints of the ensemble-reranking tests: images of 36 x 8 random features, captions from
tests/golden/g14_data_layer.npz (later passes get another line appended, so that neighbouring captions differ), models of
embed_size 32 / sim_dim 16 saved as `model_best.pth.tar` in a directory of their own."""
import os

import numpy as np
import torch

from itr_amd import config as C, utils
from itr_amd.modalmodule import get_model


def dataset(g, tmp_path, n_img, name='toy_precomp'):
    d = tmp_path / 'data' / name
    d.mkdir(parents=True)
    caps = bytes(g["caps_blob"]).split(b"\n")[:-1]
    rng = np.random.RandomState(0)
    np.save(d / 'test_ims.npy', rng.randn(n_img, 36, 8).astype(np.float32))
    lines = [caps[i % len(caps)] + (b"" if i < len(caps) else b" " + caps[(7 * i + 3 + i // len(caps)) % len(caps)]) for i in range(5 * n_img)]
    (d / 'test_caps.txt').write_bytes(b"\n".join(lines) + b"\n")
    vdir = tmp_path / 'vocab'
    vdir.mkdir(exist_ok=True)
    (vdir / ('%s_vocab.json' % name)).write_text(bytes(g["vocab_json"]).decode())
    return name, str(tmp_path / 'data'), str(vdir)


def checkpoint(g, tmp_path, tag, model_name, extra, name, data_path, vdir, seed, batch_size=7):
    save_dir = str(tmp_path / tag)
    os.makedirs(save_dir)
    cfg = C.build_config(['with', model_name, 'data_name=%s' % name, 'bi_gru=True', 'seed=%d' % seed] + extra)
    cfg.update(img_dim=8, embed_size=32, word_dim=16, vocab_size=int(g["vocab_len"]), data_path=data_path, vocab_path=vdir,
               batch_size=batch_size, workers=0, save_dir=save_dir, word_tokenize=None, sim_dim=16, vocab_type='json')
    torch.manual_seed(seed)
    model = get_model(cfg)
    utils.save_checkpoint({'epoch': 0, 'model': model.state_dict(), 'best_rsum': 0.0, 'best_r1': 0.0, '_config': cfg, 'Eiters': 1},
                          True, prefix=save_dir)
    return os.path.join(save_dir, 'model_best.pth.tar')
