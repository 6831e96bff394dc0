"""Model wrappers with the reference's interface (itr/modalmodule/Models.py): attributes config, img_enc,
txt_enc, sim_enc, criterion, optimizer, Eiters, logger; methods forward_emb / forward_loss / train_emb / val_start /
train_start / state_dict / load_state_dict.  Towers and losses run on the HIP kernels.

`train_emb` (forward -> loss -> backward -> clip_grad_norm_ -> Adam, Models.py:115-145, :198-225, :444-464) is built for the
GRU family with a pooled or SCAN similarity (VSE++, SCAN) and for SAEM (frozen BERT in training mode, cnn / pooling / trans
head and the image transformer layer on the tape, live dropout) and CAMERA (AGSA with BatchNorm batch statistics,
dilated-convolution summarisation, multi-view matching): itr_amd/autograd.py wires the HIP forward / backward kernels into
torch's tape.  SGRAF trains too: its similarity module runs the reference's per-caption structure on the tape in training
mode (Fusionmodule.encoder_similarity_train) and the fused kernels in evaluation mode; VSRN trains with its captioning branch.

Data-parallel training (the reference has none): with torch.distributed initialised and world > 1,
every rank receives the SAME global batch (loaders share the seed), keeps the strided shard rank::world of it, runs
the towers on the shard, all-gathers the caption (word) embeddings, scores its image rows against ALL captions,
all-gathers the score rows and evaluates the hinge on the full B x B matrix -- so the hardest negatives are searched
in the GLOBAL batch and the step equals the single-GPU one up to fp32 summation order.  Gradients: caption
embeddings sum-all-reduced inside the gather's backward, parameters in one flat bucket inside Adam.step."""
import numpy as np
import torch
from torch import nn

from .. import autograd as ag
from .. import ops
from . import ImgEncoder, TextEncoder, Objectives, Fusionmodule


class base_module(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        Objectives.retrieval_loss_kind(config)      # an unknown config['loss'] is refused here, when the model is built
        self.grad_clip = config.get('grad_clip', 2.)
        self.Eiters = 0
        self.img_enc = None
        self.txt_enc = None
        self.sim_enc = None
        self.criterion = None
        self.optimizer = None
        self.params = None
        self.logger = None
        self.train_im_div = None         # captions per image of the training set (train.py sets it); read by mask_same_image and memory_bank
        self.memory = None               # the cross-batch memory (membank.MemoryBank), made by the first step with memory_bank > 0
        self._xbm_pending = None         # the step's rows, pushed once its backward has run
        self._xbm_config()
        object.__setattr__(self, 'distill_teacher', None)      # a frozen fine model (attach_distill_teacher); never a registered submodule
        self._distill_config()

    def calculate_params(self):
        self.params_num = sum(p.numel() for p in self.params)
        if self.optimizer is None:       # every wrapper owns Adam(params, lr) like the reference (Models.py:98, :178)
            self.optimizer = ag.Adam(self.params, lr=self.config['learning_rate'])

    def state_dict(self):
        """List layout of the reference (Models.py:37-40).  The reference stores the sim_enc MODULE as the third
        entry; its state_dict is stored here, and load_state_dict accepts either."""
        sd = [self.img_enc.state_dict(), self.txt_enc.state_dict()]
        if self.sim_enc is not None:
            sd.append(self.sim_enc.state_dict())
        return sd

    @staticmethod
    def _strip_dp(sd):
        """The reference wraps CAMERA's towers in nn.DataParallel (Models.py:561-562), so its checkpoints name their tensors
        'module.<name>'; accepted for every model."""
        if isinstance(sd, dict) and sd and all(k.startswith('module.') for k in sd):
            return type(sd)((k[len('module.'):], v) for k, v in sd.items())
        return sd

    def load_state_dict(self, state_dict):
        self.img_enc.load_state_dict(self._strip_dp(state_dict[0]))
        self.txt_enc.load_state_dict(self._strip_dp(state_dict[1]))
        if self.sim_enc is not None:
            third = state_dict[2]
            self.sim_enc.load_state_dict(third.state_dict() if isinstance(third, nn.Module) else third)
        self._xbm_pending = None
        if self.memory is not None:      # stale embeddings belong to other weights
            self.memory.reset()

    def train_start(self):
        self.img_enc.train()
        self.txt_enc.train()
        if self.sim_enc is not None:
            self.sim_enc.train()

    def val_start(self):
        self.img_enc.eval()
        self.txt_enc.eval()
        if self.sim_enc is not None:
            self.sim_enc.eval()

    def _log(self, k, v, n=0):
        if self.logger is not None:
            self.logger.update(k, v, n)

    def train_emb(self, train_data, *a, **k):
        raise NotImplementedError("%s does not define train_emb" % type(self).__name__)      # (every model family of the reference does)

    # ---- data-parallel sharding of one global batch
    def _dp_comm(self):
        from ..evalpipe import Comm
        comm = Comm()
        if self.optimizer is not None:
            self.optimizer.comm = comm if comm.on else None
        return comm

    @staticmethod
    def _dp_shard(comm, images, captions, lengths):
        """Strided shard rank::world of a length-sorted batch (every shard stays sorted and gets the same mix of
        lengths).  Returns the shard + the rank-major global bookkeeping every rank can derive without communication:
        rows per rank, lengths of all captions in gathered order."""
        B = len(lengths)
        if B < comm.world:
            raise ValueError("data-parallel train_emb: batch of %d on %d ranks" % (B, comm.world))
        sel = [list(range(q, B, comm.world)) for q in range(comm.world)]
        mine = sel[comm.rank]
        idx = torch.as_tensor(mine, dtype=torch.long)
        lens_all = [int(lengths[i]) for q in range(comm.world) for i in sel[q]]
        rows = [len(x) for x in sel]
        toks = [sum(int(lengths[i]) for i in x) for x in sel]
        lens = [int(lengths[i]) for i in mine]
        images = images[idx.to(images.device)]
        captions = captions[idx.to(captions.device)][:, :max(lens)]
        return images, captions, lens, rows, toks, lens_all

    def _hinge(self, scores, groups):
        """The retrieval loss of a training step; `groups` from _hinge_groups (None: exactly the reference's call).
        config['loss'] = 'infonce' puts the softmax contrastive loss in the hinge's place, on the same matrix and groups."""
        if Objectives.retrieval_loss_kind(self.config) == 'infonce':
            return ops.infonce_loss(scores, self.config.get('temperature', 0.05), groups=groups)
        if groups is None:
            return ops.hinge_loss(scores, self.config['margin'], self.config['max_violation'])
        return ops.hinge_loss(scores, self.config['margin'], self.config['max_violation'], groups=groups)

    xbm_supported = False                # True in the families whose step forms scores = pair(img, cap) from two pooled matrices

    def _xbm_config(self):
        """memory_bank / memory_start are refused here, when the model is built, if they cannot mean anything."""
        cfg = self.config
        for key in ('memory_bank', 'memory_start'):
            v = cfg.get(key, 0)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError("%s must be a non-negative integer, got %r" % (key, v))
        M = cfg.get('memory_bank', 0)
        if M > 0 and not self.xbm_supported:
            raise ValueError("memory_bank=%d: %s has no cross-batch memory (VSE++, VSRN and SAEM have one: their step scores two pooled "
                             "embedding matrices; word-level and multi-view memories are not built)" % (M, type(self).__name__))
        if 0 < M < cfg.get('batch_size', 0):
            raise ValueError("memory_bank=%d is smaller than batch_size=%d: a step's rows would not fit the memory" % (M, cfg['batch_size']))

    def _hinge_memory(self, img, cap, scores, ids, pair_fn, groups=None, comm=None):
        """The retrieval loss of a step of the pooled families, `scores` = pair_fn(img, cap).  config['memory_bank'] = 0 (the
        default), or a memory not yet in use: self._hinge(scores, groups), the very call the step made before.  Otherwise every query
        also ranks against the memory: R = pair_fn(img, memory captions) and C = pair_fn(memory images, cap) go on the tape (the memory
        carries no gradient) and config['loss'] picks ops.xbm_hinge_loss or ops.xbm_infonce_loss.  The step's (img, cap) are pushed
        every step -- by _step, after the backward, because the memory's tables are operands saved on the tape."""
        M = self.config.get('memory_bank', 0)
        if not M:
            return self._hinge(scores, groups)
        if comm is not None and comm.on:
            raise ValueError("memory_bank=%d under data parallelism (%d ranks): every rank would keep its own memory of the gathered "
                             "embeddings; a memory is built for one process only" % (M, comm.world))
        if not self.train_im_div:
            raise ValueError("memory_bank=%d needs model.train_im_div, the captions per image of the training set "
                             "(train.py sets it from the dataset's im_div; 5 for the precomp splits)" % M)
        from ..membank import MemoryBank
        own = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids, dtype=np.int64).reshape(-1) // int(self.train_im_div)
        if scores.shape[0] > M:
            raise ValueError("memory_bank=%d is smaller than the batch of %d" % (M, scores.shape[0]))
        if self.memory is None or self.memory.capacity != M:
            self.memory = MemoryBank(M, scores.device)
        if self.Eiters > self.config.get('memory_start', 0) and len(self.memory) > 0:
            bank_img, bank_cap, bank_groups = self.memory.view()
            R = pair_fn(img, bank_cap)
            C = pair_fn(bank_img, cap)
            mask_batch = bool(self.config.get('mask_same_image', False))
            if Objectives.retrieval_loss_kind(self.config) == 'infonce':
                loss = ops.xbm_infonce_loss(scores, R, C, own, bank_groups, self.config.get('temperature', 0.05), mask_batch=mask_batch)
            else:
                loss = ops.xbm_hinge_loss(scores, R, C, own, bank_groups, self.config['margin'], self.config['max_violation'],
                                          mask_batch=mask_batch)
        else:
            loss = self._hinge(scores, groups)
        self._xbm_pending = (img.detach(), cap.detach(), own)
        return loss

    # ---- score distillation from a fine teacher
    distill_student = False              # True in the pooled GRU-text families that --rerank accepts as coarse (VSE++, VSRN)

    def _distill_config(self):
        """The distill_* keys are refused here, when the model is built, if they cannot mean anything.  distill_teacher = '' (the
        default, and every configuration read from an old checkpoint) is off; the teacher itself is attached after the build."""
        cfg = self.config
        w = cfg.get('distill_weight', 1.0)
        if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)) or not np.isfinite(w) or w <= 0:
            raise ValueError("distill_weight must be finite and > 0, got %r" % (w,))
        ops._distill_scale(cfg.get('distill_temperature', 0.05), "distill_temperature")
        ops._distill_scale(cfg.get('distill_teacher_temperature', 0.05), "distill_teacher_temperature")
        path = cfg.get('distill_teacher', '')
        if not isinstance(path, str):
            raise ValueError("distill_teacher must be a checkpoint path or '' (off), got %r" % (path,))
        if path:
            self._distill_student_check("distill_teacher=%r" % path)

    def _distill_student_check(self, what):
        if not self.distill_student:
            raise ValueError("%s: %s cannot be a distillation student (VSE++ and VSRN can: the pooled GRU-text models a reranking "
                             "pipeline takes as its coarse stage; SAEM / CAMERA batches carry BERT tokens, SCAN / SGRAF are teachers)"
                             % (what, type(self).__name__))
        M = self.config.get('memory_bank', 0)
        if M > 0:
            raise ValueError("%s together with memory_bank=%d: the teacher scores the batch only, not the memory" % (what, M))

    def attach_distill_teacher(self, teacher):
        """Make `teacher` (a built SCAN or SGRAF model, or None to detach) the fine model whose scores of every training batch this
        model is distilled from.  The teacher is only ever run under no_grad in evaluation mode; it is no submodule of this model and
        no part of state_dict() or of a checkpoint."""
        if teacher is not None:
            self._distill_student_check("a distillation teacher")
            name = teacher.config.get('name') if isinstance(teacher, base_module) else None
            if not isinstance(teacher, (SCAN, SGRAF)) or name not in ('SCAN', 'SGRAF'):
                raise ValueError("a distillation teacher must be a SCAN or SGRAF model, got %s" % (type(teacher).__name__,))
            for key in ('vocab_size', 'img_dim'):
                if teacher.config.get(key) != self.config.get(key):
                    raise ValueError("distillation: the teacher's %s=%r differs from the student's %s=%r: both read the same batch"
                                     % (key, teacher.config.get(key), key, self.config.get(key)))
        object.__setattr__(self, 'distill_teacher', teacher)

    def _distill(self, loss, scores, images, captions, lengths, comm):
        """`loss` (what _hinge / _hinge_memory returned) when no teacher is attached.  Otherwise the teacher scores the step's own batch
        -- evaluation mode, no_grad, forward_emb then its dense scorer (evaluation._cal_fun) -- and distill_weight * ops.distill_loss of
        the student's `scores` against them is added; the unweighted term is logged as 'Distill'."""
        teacher = self.distill_teacher
        if teacher is None:
            return loss
        if comm is not None and comm.on:
            raise ValueError("a distillation teacher under data parallelism (%d ranks): the teacher would have to score the global "
                             "batch on every rank; distillation is built for one process only" % comm.world)
        from ..metricmodule.evaluation import _cal_fun
        cfg = self.config
        teacher.val_start()
        with torch.no_grad():
            emb = teacher.forward_emb(images, captions, lengths)
            target = _cal_fun(teacher)(emb[0], emb[1], lengths, teacher.config)
        term = ops.distill_loss(scores, target.detach().to(torch.float32), cfg.get('distill_temperature', 0.05),
                                cfg.get('distill_teacher_temperature', 0.05))
        self._log('Distill', term.detach(), scores.size(0))
        return loss + cfg.get('distill_weight', 1.0) * term

    def _hinge_groups(self, ids, comm):
        """config['mask_same_image'] off (the default, and every configuration read from an old checkpoint): None.  On: the image of
        every pair, ids // train_im_div (host array), in the ROW ORDER OF THE SCORE MATRIX the step hands to the hinge -- the batch
        order in one process, and the rank-major strided order of _dp_shard (rows q, q + world, ... of rank 0, then rank 1, ...) under
        data parallelism, for every family: each shards by rank::world and gathers rank-major (SAEM's `order`, CAMERA's and VSRN's
        `sel`).  Every rank derives it from the global batch without communication, like lens_all."""
        if not self.config.get('mask_same_image', False):
            return None
        if not self.train_im_div:
            raise ValueError("mask_same_image=True needs model.train_im_div, the captions per image of the training set "
                             "(train.py sets it from the dataset's im_div; 5 for the precomp splits)")
        ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids, dtype=np.int64).reshape(-1)
        if comm.on:
            ids = np.concatenate([ids[q::comm.world] for q in range(comm.world)])
        return ids // int(self.train_im_div)

    # ---- shared by the GRU-family training steps
    def _train_towers(self, images, captions, lengths, pooled_images, last_state):
        """Differentiable towers on one batch -> (img_emb, packed word / caption embeddings, tok_off, lens).
        Same arithmetic as forward_emb; captions arrive sorted by length (collate_fn)."""
        images = self._dev(images)
        captions = self._dev(captions)
        ie, te = self.img_enc, self.txt_enc
        img = ie.forward_train(ops.mean_mid(images) if pooled_images else images)
        if getattr(te, 'dropout_p', 0.) > 0 and te.training and not hasattr(self, '_seeds'):
            self._seeds = ag.DropoutSeeds()
            self._seeds.new_step()
        if last_state != (te.method_name in ('VSE++', 'VSRN')):
            raise ValueError("_train_towers: last_state=%r does not match the text tower's pooling (method_name=%r)" % (last_state, te.method_name))
        seq, off, lens, _ = te.forward_packed_train(captions, lengths, seeds=getattr(self, '_seeds', None))
        return img, seq, off, lens

    def _step(self, loss, batch_size, logged=None):
        """backward -> clip_grad_norm_(params, grad_clip) -> Adam (Models.py:139-144, :220-225).  `logged`: the value of the
        whole batch when `loss` holds only this rank's part of a term (data parallel)."""
        self._log('Loss', loss.detach() if logged is None else logged, batch_size)      # a device scalar like the reference's loss.data: no host sync here
        loss.backward()
        if self._xbm_pending is not None:
            pending, self._xbm_pending = self._xbm_pending, None
            self.memory.push(*pending)
        self.optimizer.step(max_norm=self.grad_clip if self.grad_clip > 0 else 0.0)

    @staticmethod
    def _dev(t):
        return t.cuda() if torch.is_tensor(t) and not t.is_cuda else t


class VSE_PP(base_module):
    """VSE++ (Models.py:63-145) with the build decisions of SURVEY Q3 for *_precomp data: mean-pooled regions
    -> fc -> l2norm; text = last valid GRU state -> l2norm; honours bi_gru."""

    xbm_supported = True
    distill_student = True

    def __init__(self, config):
        super().__init__(config)
        if not config['data_name'].endswith('_precomp'):
            raise NotImplementedError("raw-image VSE++ (EncoderImageFull: torchvision CNN) is out of scope")
        self.img_enc = ImgEncoder.EncoderImagePooledPrecomp(config['img_dim'], config['embed_size'],
                                                            no_imgnorm=config['no_imgnorm'],
                                                            precomp_enc_type='basic', use_abs=config['use_abs'])
        self.txt_enc = TextEncoder.EncoderText(config['vocab_size'], config['word_dim'], config['embed_size'],
                                               config['num_layers'], use_bi_gru=config.get('bi_gru', False),
                                               use_abs=config['use_abs'], no_txtnorm=False, method_name='VSE++')
        self.img_enc.cuda()
        self.txt_enc.cuda()
        self.criterion = Objectives.make_criterion(config)
        self.params = list(self.txt_enc.parameters()) + list(self.img_enc.fc.parameters())
        self.optimizer = ag.Adam(self.params, lr=config['learning_rate'])
        self.calculate_params()

    def forward_emb(self, images, captions, lengths, *args, **kwargs):
        img_emb = self.img_enc(self._dev(images))
        cap_emb, _ = self.txt_enc(self._dev(captions), lengths)
        return img_emb, cap_emb

    def train_emb(self, train_data, *args, **kwargs):
        """One training step (Models.py:115-145)."""
        images, _, _, captions, lengths, ids, _, _ = train_data
        if self.config['measure'] not in ('cosine', 'order'):
            raise ValueError("unknown measure:", self.config['measure'])
        pair_scores = ag.order_scores if self.config['measure'] == 'order' else ag.cosine_scores
        self.Eiters += 1
        self._log('Eit', self.Eiters)
        self._log('lr', self.optimizer.param_groups[0]['lr'])
        self.optimizer.zero_grad()
        comm = self._dp_comm()
        groups = self._hinge_groups(ids, comm)
        if comm.on:
            images, captions, lengths, rows, _, _ = self._dp_shard(comm, images, captions, lengths)
        with torch.enable_grad():
            img, cap, _, _ = self._train_towers(images, captions, lengths, pooled_images=True, last_state=True)
            if comm.on:
                cap = ag.dp_gather_rows(cap, comm, rows, reduce=True)
                scores = ag.dp_gather_rows(pair_scores(img, cap), comm, rows, reduce=False)
            else:
                scores = pair_scores(img, cap)
            loss = self._hinge_memory(img, cap, scores, ids, pair_scores, groups, comm)
            loss = self._distill(loss, scores, images, captions, lengths, comm)
            self._step(loss, scores.size(0))

    def forward_loss(self, img_emb, cap_emb):
        loss = self.criterion(img_emb, cap_emb)
        self._log('Loss', loss.data, img_emb.size(0))
        return loss


class SCAN(base_module):
    """Stacked Cross Attention Network (Models.py:148-225)."""

    def __init__(self, config):
        super().__init__(config)
        self.img_enc = ImgEncoder.EncoderImagePrecomp(config['img_dim'], config['embed_size'],
                                                      precomp_enc_type=config['precomp_enc_type'],
                                                      no_imgnorm=config['no_imgnorm'])
        self.txt_enc = TextEncoder.EncoderText(config['vocab_size'], config['word_dim'], config['embed_size'],
                                               config['num_layers'], use_bi_gru=config['bi_gru'],
                                               no_txtnorm=config['no_txtnorm'])
        self.img_enc.cuda()
        self.txt_enc.cuda()
        self.criterion = Objectives.make_criterion(config)
        self.params = list(self.txt_enc.parameters()) + list(self.img_enc.fc.parameters())
        self.optimizer = ag.Adam(self.params, lr=config['learning_rate'])
        self.calculate_params()

    def forward_emb(self, images, captions, lengths, *args, **kwargs):
        img_emb = self.img_enc(self._dev(images))
        cap_emb, cap_lens = self.txt_enc(self._dev(captions), lengths)
        return img_emb, cap_emb, cap_lens

    def train_emb(self, train_data, *args, **kwargs):
        """One training step (Models.py:198-225)."""
        images, _, _, captions, lengths, ids, _, _ = train_data
        cfg = self.config
        if cfg['cross_attn'] not in ('t2i', 'i2t'):
            raise ValueError("unknown first norm type:", cfg['raw_feature_norm'])
        self.Eiters += 1
        self._log('Eit', self.Eiters)
        self._log('lr', self.optimizer.param_groups[0]['lr'])
        self.optimizer.zero_grad()
        comm = self._dp_comm()
        groups = self._hinge_groups(ids, comm)
        if comm.on:
            images, captions, lengths, rows, toks, lens_all = self._dp_shard(comm, images, captions, lengths)
        with torch.enable_grad():
            img, words, off, lens = self._train_towers(images, captions, lengths, pooled_images=False, last_state=False)
            if comm.on:
                words = ag.dp_gather_rows(words, comm, toks, reduce=True)
                lens = lens_all
                off = np.concatenate([[0], np.cumsum(lens_all)[:-1]]).astype(np.int64)
            score_fn = ag.scan_t2i_scores if cfg['cross_attn'] == 't2i' else ag.scan_i2t_scores
            scores = score_fn(img, words, off, lens, cfg['raw_feature_norm'], cfg['agg_func'], cfg['lambda_lse'], cfg['lambda_softmax'])
            if comm.on:
                scores = ag.dp_gather_rows(scores, comm, rows, reduce=False)
            loss = self._hinge(scores, groups)
            self._step(loss, scores.size(0))

    def forward_loss(self, img_emb, cap_emb, cap_lens):
        loss = self.criterion(img_emb, cap_emb, cap_lens)
        self._log('Loss', loss.data, img_emb.size(0))
        return loss


class VSRN(base_module):
    """Visual Semantic Reasoning Network (Models.py:229-365): region-relationship GCN + region GRU image tower, last-state GRU text
    tower, cosine similarity, plus the training-only captioning branch (EncoderRNN / attention DecoderRNN over the GCN region
    features, LanguageModelCriterion).  The reference's checkpoints hold [img_enc, txt_enc] only (Models.py:37-45: the captioning
    model is never saved) -- the same here."""

    xbm_supported = True
    distill_student = True

    def __init__(self, config, use_txt_emb=True):
        super().__init__(config)
        if not config['data_name'].endswith('_precomp'):
            raise NotImplementedError("raw-image VSRN (EncoderImageFull: torchvision CNN) is out of scope")
        if use_txt_emb:
            self.img_enc = ImgEncoder.EncoderImagePrecompAttn(config['img_dim'], config['embed_size'], config['data_name'],
                                                              use_abs=config['use_abs'], no_imgnorm=config['no_imgnorm'])
        else:
            self.img_enc = ImgEncoder.EncoderImagePrecomp(config['img_dim'], config['embed_size'], use_abs=config['use_abs'],
                                                          no_imgnorm=config['no_imgnorm'])
        self.txt_enc = TextEncoder.EncoderText(config['vocab_size'], config['word_dim'], config['embed_size'],
                                               config['num_layers'], use_abs=config['use_abs'],
                                               no_txtnorm=config['no_txtnorm'], method_name=config['name'])
        self.encoder = Fusionmodule.EncoderRNN(config['dim_vid'], config['dim_hidden'], bidirectional=config['bidirectional'],
                                               input_dropout_p=config['input_dropout_p'], rnn_cell=config['rnn_type'],
                                               rnn_dropout_p=config['rnn_dropout_p'])
        self.decoder = Fusionmodule.DecoderRNN(config['vocab_size'], config['max_len'], config['dim_hidden'], config['dim_word'],
                                               input_dropout_p=config['input_dropout_p'], rnn_cell=config['rnn_type'],
                                               rnn_dropout_p=config['rnn_dropout_p'], bidirectional=config['bidirectional'])
        self.caption_model = Fusionmodule.S2VTAttModel(self.encoder, self.decoder)
        self.img_enc.cuda()
        self.txt_enc.cuda()
        self.caption_model.cuda()
        self.criterion = Objectives.make_criterion(config)
        self.params = list(self.txt_enc.parameters()) + list(self.img_enc.parameters()) + list(self.caption_model.parameters())
        self.calculate_params()

    def train_start(self):
        super().train_start()
        self.caption_model.train()

    def val_start(self):
        super().val_start()
        self.caption_model.eval()

    def forward_emb(self, images, captions, lengths, *args, **kwargs):
        out = self.img_enc(self._dev(images))
        img_emb, gcn_emb = out if isinstance(out, tuple) else (out, None)
        cap_emb, _ = self.txt_enc(self._dev(captions), lengths)
        return img_emb, cap_emb, gcn_emb

    def forward_loss(self, img_emb, cap_emb, GCN_img_emd=None, captions=None, captions_mask=None):
        """Retrieval loss (Models.py:337) on evaluation-mode embeddings.  The captioning term needs the autograd tape through the
        towers: it is part of train_emb (passing captions here raises)."""
        if captions is not None:
            raise NotImplementedError("the captioning loss is evaluated inside train_emb (the towers must be on the autograd tape)")
        loss = self.criterion(img_emb, cap_emb)
        self._log('Loss_retrieval', loss.data, img_emb.size(0))
        self._log('Loss', loss.data, img_emb.size(0))
        return loss

    def train_emb(self, train_data, *args, **kwargs):
        """One training step (Models.py:343-365): towers on the autograd tape -> retrieval hinge + captioning loss
        (calcualte_caption_loss :303-313) -> backward, clip_grad_norm_, Adam."""
        images, _, _, captions, lengths, ids, captions_mask, _ = train_data
        if not isinstance(self.img_enc, ImgEncoder.EncoderImagePrecompAttn):
            raise NotImplementedError("VSRN.train_emb with use_txt_emb=False")
        if self.config['measure'] not in ('cosine', 'order'):
            raise ValueError("unknown measure:", self.config['measure'])
        self.Eiters += 1
        self._log('Eit', self.Eiters)
        self._log('lr', self.optimizer.param_groups[0]['lr'])
        if not hasattr(self, '_seeds'):
            self._seeds = ag.DropoutSeeds()
        self._seeds.new_step()
        comm = self._dp_comm()
        groups = self._hinge_groups(ids, comm)
        n_batch = len(lengths)
        if comm.on:
            # data parallel: a strided shard through the towers (the BatchNorms of the GCN and of the image tower take their
            # statistics over the rows of all ranks, ag.bn_sync), embeddings all-gathered, retrieval hinge replicated on the full
            # batch; the captioning loss is a sum over rows / batch size, so every rank adds its shard's part of it
            if n_batch < comm.world:
                raise ValueError("data-parallel train_emb: batch of %d on %d ranks" % (n_batch, comm.world))
            sel = torch.arange(comm.rank, n_batch, comm.world)
            rows = [len(range(q, n_batch, comm.world)) for q in range(comm.world)]
            images, captions, captions_mask = (t[sel.to(t.device)] for t in (images, captions, captions_mask))
            lengths = [lengths[i] for i in sel.tolist()]
            self._seeds.base += comm.rank * 7919                                                # other masks on other shards
        self.optimizer.zero_grad()
        with torch.enable_grad(), ag.bn_sync(comm):
            images, captions = self._dev(images), self._dev(captions)
            img, gcn_emb = self.img_enc.forward_train(images)
            te = self.txt_enc
            toks, off, lens, _ = TextEncoder.pack_tokens(captions, lengths)
            seq = ag.gru_sequence(toks, off, lens, te.embed.weight, dict(te.rnn.named_parameters()), te.use_bi_gru)
            cap = ag.gather_rows(seq, off + ops.h2d(np.asarray(lens, np.int64), off.device) - 1)
            if not te.no_txtnorm:
                cap = ag.l2norm_rows(cap)
            if te.use_abs:
                cap = cap.abs()
            if comm.on:
                img = ag.dp_gather_rows(img, comm, rows, reduce=False)
                cap = ag.dp_gather_rows(cap, comm, rows, reduce=False)
            pair_scores = ag.order_scores if self.config['measure'] == 'order' else ag.cosine_scores
            scores = pair_scores(img, cap)
            retrieval_loss = self._hinge_memory(img, cap, scores, ids, pair_scores, groups, comm)
            retrieval_loss = self._distill(retrieval_loss, scores, images, captions, lengths, comm)
            caption_loss = self.caption_model.caption_loss_train(gcn_emb, captions, self._dev(captions_mask), self._seeds,
                                                                 self.caption_model.training, batch_total=n_batch)
            caption_total = caption_loss.detach()
            if comm.on:
                import torch.distributed as dist
                caption_total = comm.all_reduce(caption_total.clone(), dist.ReduceOp.SUM)          # for the log only
            self._log('Loss_caption', caption_total, img.size(0))
            self._log('Loss_retrieval', retrieval_loss.detach(), img.size(0))
            self._step(retrieval_loss + caption_loss, img.size(0), logged=retrieval_loss.detach() + caption_total)


class SGRAF(base_module):
    """Similarity Reasoning and Filtration network (Models.py:468-546)."""

    def __init__(self, config):
        super().__init__(config)
        self.img_enc = ImgEncoder.EncoderImagePrecomp(config['img_dim'], config['embed_size'],
                                                      no_imgnorm=config['no_imgnorm'], precomp_enc_type='basic')
        self.txt_enc = TextEncoder.EncoderText(config['vocab_size'], config['word_dim'], config['embed_size'],
                                               config['num_layers'], use_bi_gru=config['bi_gru'],
                                               no_txtnorm=config['no_txtnorm'], dropout=.4)
        self.sim_enc = Fusionmodule.EncoderSimilarity(config['embed_size'], config['sim_dim'], config['module_name'],
                                                      config['sgr_step'])
        self.img_enc.cuda()
        self.txt_enc.cuda()
        self.sim_enc.cuda()
        self.criterion = Objectives.make_criterion(config)
        self.params = list(self.txt_enc.parameters()) + list(self.img_enc.parameters()) + list(self.sim_enc.parameters())
        self.calculate_params()

    def forward_emb(self, images, captions, lengths, *args, **kwargs):
        img_embs = self.img_enc(self._dev(images))
        cap_embs, _ = self.txt_enc(self._dev(captions), lengths)
        return img_embs, cap_embs

    def forward_loss(self, sims):
        loss = self.criterion(sims)
        self._log('Loss', loss.item(), sims.size(0))
        return loss

    def train_emb(self, train_data, *args, **kwargs):
        """One training step (Models.py:524-546): towers and the similarity module on the autograd tape (word-embedding and
        self-attention dropout live, BatchNorm batch statistics), hinge on the B x B similarity matrix, backward,
        clip_grad_norm_, Adam.  The similarity module follows the reference's per-caption structure in training mode
        (Fusionmodule.encoder_similarity_train); evaluation uses the fused kernels."""
        images, _, _, captions, lengths, ids, _, _ = train_data
        self.Eiters += 1
        self._log('Eit', self.Eiters)
        self._log('lr', self.optimizer.param_groups[0]['lr'])
        if not hasattr(self, '_seeds'):
            self._seeds = ag.DropoutSeeds()
        self._seeds.new_step()
        self.optimizer.zero_grad()
        comm = self._dp_comm()
        groups = self._hinge_groups(ids, comm)
        shared = None
        if comm.on:
            # data parallel by CAPTION (the similarity module works caption by caption, each against all images): towers on a
            # strided shard, region embeddings all-gathered (every rank holds a partial gradient for all of them: summed in the
            # gather's backward), this rank's columns of the B x B matrix, columns all-gathered, hinge replicated.  The global
            # image vectors (VisualSA: BatchNorm over the image batch) are computed replicated on the gathered embeddings with the
            # same dropout masks everywhere; all other dropout sites draw other masks on other shards.
            images, captions, lengths, rows, _, _ = self._dp_shard(comm, images, captions, lengths)
            shared = ag.DropoutSeeds()
            shared.base, shared.n = self._seeds.base, 2048
            self._seeds.base += comm.rank * 7919
        with torch.enable_grad():
            img, words, off, lens = self._train_towers(images, captions, lengths, pooled_images=False, last_state=False)
            if comm.on:
                img = ag.dp_gather_rows(img, comm, rows, reduce=True)
            off_host = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            sims = Fusionmodule.encoder_similarity_train(self.sim_enc, img, words, off_host, [int(x) for x in lens], self._seeds,
                                                         self.sim_enc.training, seeds_global=shared)
            if comm.on:
                sims = ag.dp_gather_rows(sims.t().contiguous(), comm, rows, reduce=False).t()      # (images, captions), both rank-major
            loss = self._hinge(sims, groups)
            self._step(loss, sims.size(0))


class SAEM(base_module):
    """SAEM (Models.py:369-464): BERT text tower + transformer image tower, cosine via pdist_cos."""

    xbm_supported = True

    def __init__(self, config):
        super().__init__(config)
        self.img_enc = ImgEncoder.TransformerMapping(config)
        self.txt_enc = TextEncoder.BertMapping(config)
        self.txt_enc.cuda()
        self.img_enc.cuda()
        self.criterion = Objectives.make_criterion(config)
        self.criterion_2 = Objectives.AngularLoss()
        self.params = list(self.txt_enc.parameters()) + list(self.img_enc.parameters())
        self.calculate_params()
        # Adam over the parameters that receive gradients (the reference hands the frozen BERT weights to Adam as well; they
        # never get a gradient there either)
        self.optimizer = ag.Adam([p_ for p_ in self.params if p_.requires_grad], lr=config['learning_rate'])
        self.no_decay = ['bias', 'gamma', 'beta']

    def forward_emb(self, images, captions, captions_mask, captions_type_ids, lengths, *args, **kwargs):
        cap_embs = self.txt_enc(self._dev(captions), self._dev(captions_mask), self._dev(captions_type_ids), lengths)
        img_embs = self.img_enc(self._dev(images))
        return img_embs, cap_embs

    def forward_loss(self, epoch, img_emb, cap_emb, cap_len, ids):
        """loss1 + alpha(epoch) * AngularLoss + 0.01 * sum ||W|| over the image tower's decayed parameters
        (Models.py:419-442).  The ranking term runs on the HIP kernels; the two auxiliaries are training-time scalars
        composed of torch GPU ops."""
        alpha = 0 if epoch > 20 else 0.5 * (0.1 ** (epoch // 5))
        loss1 = self.criterion(img_emb, cap_emb, cap_len)
        loss2 = self.criterion_2(img_emb, cap_emb, cap_len, ids)
        self._log('Loss1', loss1.item(), img_emb.size(0))
        self._log('Loss2', loss2.item(), img_emb.size(0))
        l2_reg = torch.zeros((), device=img_emb.device)
        for name, param in self.img_enc.named_parameters():
            if name.split('.')[-1] not in self.no_decay:
                l2_reg = l2_reg + torch.norm(param.detach())
        return loss1 + alpha * loss2 + 0.01 * l2_reg

    def train_emb(self, train_data, epoch=0):
        """One training step (Models.py:444-464): towers on the autograd tape (frozen BERT forward in training mode, head
        and image transformer layer differentiable), loss1 + alpha(epoch) * AngularLoss + 0.01 * sum ||W||, backward,
        clip_grad_norm_, Adam.  utils.train_step never passes the epoch, so alpha is 0.5 there, as in the reference.
        mask_same_image masks the retrieval hinge (loss1) only: the angular term also takes the other rows of the batch as
        negatives, and its kernel (csrc/aux_loss.hip) has no mask -- it is left as the reference computes it."""
        images, _, _, captions, lengths, ids, captions_mask, captions_type_ids = train_data
        self.Eiters += 1
        self._log('Eit', self.Eiters)
        self._log('lr', self.optimizer.param_groups[0]['lr'])
        if not hasattr(self, '_seeds'):
            self._seeds = ag.DropoutSeeds()
        self._seeds.new_step()
        comm = self._dp_comm()
        groups = self._hinge_groups(ids, comm)          # (in the gathered order: the same permutation as ids_all below)
        rows = None
        if comm.on:
            # data parallel: strided shard of the global batch through the towers, both embedding sets all-gathered; every
            # loss term is then evaluated replicated on the full batch, so the gathers' backward is a plain slice and only the
            # parameter gradients are summed (Adam.step).  The regulariser depends on the parameters alone: 1 / world of it
            # per rank.
            B = len(lengths)
            if B < comm.world:
                raise ValueError("data-parallel train_emb: batch of %d on %d ranks" % (B, comm.world))
            sel = torch.arange(comm.rank, B, comm.world)
            rows = [len(range(q, B, comm.world)) for q in range(comm.world)]
            order = [i for q in range(comm.world) for i in range(q, B, comm.world)]          # rank-major global order
            images, captions, captions_mask, captions_type_ids = (t[sel.to(t.device)] for t in (images, captions, captions_mask, captions_type_ids))
            lengths_all, ids_all = [lengths[i] for i in order], [ids[i] for i in order]
            lengths = [lengths[i] for i in sel.tolist()]
            self._seeds.base += comm.rank * 7919                                                # other masks on other shards
        self.optimizer.zero_grad()
        with torch.enable_grad():
            cap = self.txt_enc.forward_train(self._dev(captions), self._dev(captions_mask), self._dev(captions_type_ids), lengths, self._seeds)
            img = self.img_enc.forward_train(self._dev(images), self._seeds)
            if comm.on:
                img = ag.dp_gather_rows(img, comm, rows, reduce=False)
                cap = ag.dp_gather_rows(cap, comm, rows, reduce=False)
                lengths, ids = lengths_all, ids_all
            # criterion = hinge on pdist_cos (Objectives.py:310-323: rows renormalised, no eps), on the tape
            img_n, cap_n = ag.l2norm_rows(img, eps=0.0), ag.l2norm_rows(cap, eps=0.0)
            scores = ag.cosine_scores(img_n, cap_n)
            loss1 = self._hinge_memory(img_n, cap_n, scores, ids, ag.cosine_scores, groups, comm)
            alpha = 0 if epoch > 20 else 0.5 * (0.1 ** (epoch // 5))
            loss2 = self.criterion_2(img, cap, lengths, ids)
            l2_reg = torch.zeros((), device=img.device)
            for name, param in self.img_enc.named_parameters():
                if name.split('.')[-1] not in self.no_decay:
                    l2_reg = l2_reg + torch.norm(param)
            loss = loss1 + alpha * loss2 + (0.01 / comm.world) * l2_reg
            self._log('Loss1', loss1.detach(), img.size(0))
            self._log('Loss2', loss2.detach(), img.size(0))
            self._step(loss, img.size(0))


class CAMERA(base_module):
    """CAMERA (Models.py:550-645): multi-view image embeddings (k x D per image), BERT + AGSA caption embedding,
    MultiViewMatching similarity, TripletLoss."""

    def __init__(self, config):
        super().__init__(config)
        self.img_enc = ImgEncoder.EncoderImagePrecompSelfAttn(config['img_dim'], config['embed_size'], config['head'],
                                                              config['smry_k'], drop=config['drop'])
        self.txt_enc = TextEncoder.CAMERAEncoderText(config['bert_config_file'], config['init_checkpoint'],
                                                     config['embed_size'], config['head'], drop=config['drop'])
        self.mvm = Fusionmodule.MultiViewMatching()
        self.img_enc.cuda()       # one process per GPU: no nn.DataParallel wrapper (Models.py:561-562)
        self.txt_enc.cuda()
        self.crit_ranking = Objectives.make_scores_criterion(config)
        self.crit_div = Objectives.DiversityRegularization(config['smry_k'], config['batch_size'])
        self.params = list(self.txt_enc.parameters()) + list(self.img_enc.parameters())
        self.calculate_params()
        self.optimizer = ag.Adam([p_ for p_ in self.params if p_.requires_grad], lr=config['learning_rate'])   # (frozen BERT: no gradients)

    def state_dict(self):
        """[img_enc, txt_enc] with the 'module.' prefix of the reference's nn.DataParallel wrappers (Models.py:561-562), so that a
        checkpoint written here loads in the reference on a GPU host and vice versa (load_state_dict accepts both spellings)."""
        from collections import OrderedDict
        return [OrderedDict(('module.' + k, v) for k, v in m.state_dict().items()) for m in (self.img_enc, self.txt_enc)]

    def forward_emb(self, images, boxes, imgs_wh, captions, captions_mask, captions_type_ids, *args, **kwargs):
        cap_emb = self.txt_enc(self._dev(captions), self._dev(captions_mask), self._dev(captions_type_ids))
        img_emb, smry_mat = self.img_enc(self._dev(images), self._dev(boxes), self._dev(imgs_wh))
        return img_emb, cap_emb, smry_mat

    def forward_loss(self, sim_mat, smry_mat):
        """ranking loss + smry_lamda * diversity regulariser (Models.py:598-611)."""
        ranking_loss = self.crit_ranking(sim_mat)
        self._log('Rank_Loss', ranking_loss.item(), len(sim_mat))
        div_reg = self.crit_div(smry_mat)
        self._log('Div_loss', div_reg.item(), len(sim_mat))
        loss = ranking_loss + div_reg * self.config['smry_lamda']
        self._log('Loss', loss.item(), len(sim_mat))
        return loss

    def train_emb(self, train_data, *args, **kwargs):
        """One training step (Models.py:613-645): towers on the autograd tape (frozen BERT forward in training mode, AGSA with
        BatchNorm batch statistics, dilated-convolution summarisation), multi-view matching, bidirectional hinge + smry_lamda *
        diversity regulariser, backward, clip_grad_norm_, Adam."""
        images, boxes, imgs_wh, captions, _, ids, captions_mask, captions_type_ids = train_data
        self.Eiters += 1
        self._log('Eit', self.Eiters)
        self._log('lr', self.optimizer.param_groups[0]['lr'])
        if not hasattr(self, '_seeds'):
            self._seeds = ag.DropoutSeeds()
        self._seeds.new_step()
        comm = self._dp_comm()
        groups = self._hinge_groups(ids, comm)
        if comm.on:
            # data parallel (like SAEM): a strided shard of the global batch through the towers -- every BatchNorm inside takes
            # its statistics over the rows of ALL ranks (ag.bn_sync: one small all-reduce each way) -- then the multi-view
            # embeddings, caption embeddings and summarisation matrices are all-gathered and the loss is evaluated replicated on
            # the full batch, so the gathers' backward is a slice and only the parameter gradients are summed (Adam.step)
            B = len(captions)
            if B < comm.world:
                raise ValueError("data-parallel train_emb: batch of %d on %d ranks" % (B, comm.world))
            sel = torch.arange(comm.rank, B, comm.world)
            rows = [len(range(q, B, comm.world)) for q in range(comm.world)]
            images, boxes, imgs_wh, captions, captions_mask, captions_type_ids = (
                t[sel.to(t.device)] for t in (images, boxes, imgs_wh, captions, captions_mask, captions_type_ids))
            self._seeds.base += comm.rank * 7919                                                # other masks on other shards
        self.optimizer.zero_grad()
        with torch.enable_grad(), ag.bn_sync(comm):
            cap = self.txt_enc.forward_train(self._dev(captions), self._dev(captions_mask), self._dev(captions_type_ids), self._seeds)
            img, smry_mat = self.img_enc.forward_train(self._dev(images), self._dev(boxes), self._dev(imgs_wh), self._seeds)
            if comm.on:
                img = ag.dp_gather_rows(img, comm, rows, reduce=False)
                cap = ag.dp_gather_rows(cap, comm, rows, reduce=False)
                smry_mat = ag.dp_gather_rows(smry_mat, comm, rows, reduce=False)
            sim_mat = ag.mvm_scores(img, cap)
            ranking_loss = self._hinge(sim_mat, groups)
            div_reg = self.crit_div(smry_mat)
            loss = ranking_loss + div_reg * self.config['smry_lamda']
            self._log('Rank_Loss', ranking_loss.detach(), len(sim_mat))
            self._log('Div_loss', div_reg.detach(), len(sim_mat))
            self._step(loss, len(sim_mat))
