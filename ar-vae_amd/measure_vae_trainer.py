"""MeasureVAETrainer: the AR-VAE loss step for 24-tick music measures on the HIP kernels.

Loss recipe and API of the reference's measurevae/measure_vae_trainer.py:23-186,399-400:
    loss = CE_mean(weights, score) + beta*|KL| + sum_{d in reg_dim} gamma * reg(z[:,d], attr[:,d])
The four attribute labels (rhythmic complexity, pitch range, note density, contour) come from one integer
kernel over the score batch instead of B x 24 Python loops with music21 lookups
(data/dataloaders/bar_dataset.py:338-500).
"""
from typing import Tuple

import numpy as np
import torch

from . import ops
from .midi import NON_NOTES as _NON_NOTES, pitch_to_midi      # (plain Python: the MIDI reader needs both without torch)
from .trainer import Trainer

MUSIC_REG_TYPE = {'rhy_complexity': 0, 'pitch_range': 1, 'note_density': 2, 'contour': 3}

# reference data/dataloaders/bar_dataset_helpers.py:21-30
RHY_COMPLEXITY_COEFFS = [0.20, 1, 2, 0.5, 2, 1, 0.67, 1, 2, 0.5, 2, 1, 0.25, 1, 2, 0.5, 2, 1, 0.67, 1, 2, 0.5, 2, 1]
_PADDING_SYMBOLS = ('START', 'END', None, 'None')        # vocabulary entries that are not music: never part of a playable measure


def build_measure_tables(dataset, device):
    """(midi int32[V], is_note uint8[V], is_density_note uint8[V]) from the dataset's index2note dict."""
    index2note = dataset.index2note_dicts
    v = len(index2note)
    midi, is_note, is_dens = np.zeros(v, np.int32), np.zeros(v, np.uint8), np.zeros(v, np.uint8)
    for i, sym in index2note.items():
        if sym in _NON_NOTES:
            is_dens[i] = 1 if sym is None else 0          # note density does not exclude `None` (bar_dataset.py:348-356)
            continue
        midi[i] = pitch_to_midi(sym)
        is_note[i] = is_dens[i] = 1
    return tuple(torch.from_numpy(a).to(device) for a in (midi, is_note, is_dens))


class MeasureVAETrainer(Trainer):
    def __init__(self, dataset, model, lr=1e-4, reg_type: Tuple[str] = None, reg_dim: Tuple[int] = 0, beta=0.001,
                 gamma=1.0, capacity=0.0, rand=0, delta=10.0):
        super().__init__(dataset, model, lr)
        kind = dataset.class_name[5:9]
        if kind == 'Chor':
            self.dataset_type = 'bach'
        elif kind == 'Folk':
            self.dataset_type = 'folk'
        else:
            raise ValueError('Dataset Type not recognized')
        self.attr_dict = MUSIC_REG_TYPE
        self.reverse_attr_dict = {v: k for k, v in self.attr_dict.items()}
        self.metrics = {}
        self.beta = beta
        self.capacity = torch.tensor([capacity], dtype=torch.float32)
        self.gamma = 0.0
        self.delta = 0.0
        self.cur_epoch_num = 0
        self.warm_up_epochs = 10
        self.reg_type = reg_type if reg_type is not None else ()
        self.reg_dim = ()
        self.use_reg_loss = False
        self.rand_seed = rand
        ops.rng_reseed(self.rand_seed)                 # torch.manual_seed + restart of the library's Philox stream position
        np.random.seed(self.rand_seed)
        self.trainer_config = f'_r_{self.rand_seed}_b_{self.beta}_'
        if capacity != 0.0:
            self.trainer_config += f'c_{capacity}_'
        if len(self.reg_type) != 0:
            self.use_reg_loss = True
            self.reg_dim = reg_dim
            self.gamma = gamma
            self.delta = delta
            self.trainer_config += f'g_{self.gamma}_d_{self.delta}_' + '_'.join(self.reg_type) + '_'
        self.model.update_trainer_config(self.trainer_config)
        self._tables = None
        self.last_terms = {}
        self.use_graph_replay = True          # about a hundred small launches per step: replayed from HIP graphs (trainer.py)
        # forward + loss terms and backward as one library call each (fused_measure.py, csrc/plan_measure.hip) where the executor
        # is built for the model; False keeps the per-layer autograd path (the same launches issued one by one)
        self.use_fused_step = True
        self._fused = None

    def process_batch_data(self, batch):
        score, metadata = batch
        n_bars = getattr(self.dataset, 'n_bars', None)
        if n_bars is not None:
            b = score.size(0)
            score = score.view(b * n_bars, -1)
            metadata = metadata.view(b * n_bars, -1)
        dev = next(self.model.parameters()).device
        return score.to(dev, torch.int64).contiguous(), metadata.to(dev, torch.int64).contiguous()

    def _attr_tables(self, device):
        if self._tables is None or self._tables[0][0].device != device:
            w = torch.tensor(RHY_COMPLEXITY_COEFFS, dtype=torch.float64).float()
            self._tables = (build_measure_tables(self.dataset, device), w.to(device), float(w.sum()))
        return self._tables

    def compute_attribute_labels(self, score, attr_list=None):
        """(B, 24) int64 -> (B, len(attr_list)) attribute values (all four by default)."""
        tables, w, norm = self._attr_tables(score.device)
        labels = ops.measure_attributes(score, tables, w, norm)
        if attr_list is None:
            return labels
        cols = []
        for name in attr_list:
            if name not in self.attr_dict:
                raise ValueError('Invalid regularization attribute')
            cols.append(self.attr_dict[name])
        return labels[:, cols]

    def _fused_binding(self):
        """the whole-model executor bound to this trainer's arena and hyper-parameters, or None when the steps take the per-layer
        path: debug checks, CPU models, unsupported shapes.  Data-parallel steps run it too (forward, one grouped all-gather of z
        and the attribute labels, arvae_measure_vae_finish)."""
        if not self.use_fused_step or ops.checks_enabled():
            return None
        if self.use_reg_loss and type(self.reg_dim) != tuple:
            return None                                            # (the per-layer path raises the reference's TypeError)
        from .fused_measure import FusedMeasureVAE
        from .measure_vae import _use_sequence_kernels
        reg_dims = tuple(self.reg_dim) if self.use_reg_loss else ()
        key = (reg_dims, float(self.beta), float(self.gamma), float(self.delta), self.model.decoder.sampling)
        if self._fused is None or self._fused[0] != key:
            usable = (_use_sequence_kernels(self.model.encoder.rnn_hidden_size) and next(self.model.parameters()).is_cuda
                      and FusedMeasureVAE.supports(self.model, self.optimizer, reg_dims) is None)
            self._fused = (key, FusedMeasureVAE(self.model, self.optimizer, reg_dims, self.beta, self.gamma, self.delta) if usable else None)
        return self._fused[1]

    def fused_executor(self, score):
        """-> the executor for a step on `score` (B, 24), or None: this step takes the per-layer path"""
        fused = self._fused_binding() if score.is_cuda else None
        if fused is None or not fused.fits(score.shape[0]):
            return None
        enc, dec = self.model.encoder, self.model.decoder
        if bool(enc._mask_queue) != bool(dec._mask_queue):
            return None                                            # explicit keep-masks for one half only: per-layer path
        return fused

    def _replay_step(self, batch):
        # the executor issues a step's launches from two library calls (three and one collective under data parallelism): a captured
        # graph has no host work left to save and its nodes cost more than the stream launches they replace (B = 256: 1.09 ms eager,
        # 1.11 ms replayed)
        fused = self._fused_binding()
        if fused is not None:
            score = batch[0]
            rows = score.shape[0] * (getattr(self.dataset, 'n_bars', None) or 1) if torch.is_tensor(score) else -1
            if rows > 0 and fused.fits(rows):
                return None
        return super()._replay_step(batch)                   # (a batch the executor does not take: the per-layer path, replayed)

    def _fused_loss_and_acc(self, fused, score, epoch_num, first_of_epoch, train):
        from .fused_measure import ACC, DIST, RECON, REG
        enc, dec = self.model.encoder, self.model.decoder
        eps = enc._eps_queue.popleft() if enc._eps_queue else enc.static_eps
        masks = None
        if self.model.training and enc._mask_queue:
            masks = (enc._mask_queue.popleft(),) + tuple(dec._mask_queue.popleft())
        tables = fused.tables(self, score.device) if self.use_reg_loss else None
        loss, scalars, accuracy, *_ = fused.run(score, train, None, tables, eps, masks, self.data_parallel)
        self.last_terms = {'recons': scalars[RECON], 'dist': scalars[DIST], 'reg': scalars[REG] if self.use_reg_loss else None}
        if first_of_epoch and self.writer is not None and not torch.cuda.is_current_stream_capturing():
            self.log_loss_split(epoch_num)
        return loss.reshape(()), accuracy

    def loss_and_acc_for_batch(self, batch, epoch_num=None, batch_num=None, train=True):
        first_of_epoch = self.cur_epoch_num != epoch_num
        if first_of_epoch:
            self.cur_epoch_num = epoch_num
        score, metadata = batch
        fused = self.fused_executor(score)
        if fused is not None:
            return self._fused_loss_and_acc(fused, score, epoch_num, first_of_epoch, train)
        weights, samples, z_dist, prior_dist, z_tilde, _ = self.model(measure_score_tensor=score, measure_metadata_tensor=metadata,
                                                                       train=train, need_prior_sample=False)
        recons_loss, accuracy = ops.token_recon(weights, score)
        dist_loss = self.compute_kld_loss(z_dist, prior_dist, self.beta)
        loss = recons_loss + dist_loss
        reg_loss = None
        if self.use_reg_loss:
            if type(self.reg_dim) != tuple:
                raise TypeError('Regularization dimension must be a tuple of integers')
            attr_labels = self.compute_attribute_labels(score)
            if self.data_parallel is not None:
                reg_loss = self.data_parallel.reg_loss(z_tilde, attr_labels, self.reg_dim, self.gamma, self.delta)
            else:
                reg_loss = ops.reg_loss(z_tilde, attr_labels, self.reg_dim, self.gamma, self.delta)
            loss = loss + reg_loss
        self.last_terms = {'recons': recons_loss.detach(), 'dist': dist_loss.detach(),
                           'reg': None if reg_loss is None else reg_loss.detach()}
        if first_of_epoch and self.writer is not None and not torch.cuda.is_current_stream_capturing():
            self.log_loss_split(epoch_num)
        return loss, accuracy

    def log_loss_split(self, epoch_num):
        """the loss terms of the last step to the summary writer (measure_vae_trainer.py:116-127); also called by the
        epoch loop after the first graph-replayed step of an epoch, whose terms live in the captured step's outputs."""
        t = self.last_terms
        if self.writer is None or not t:
            return
        self.writer.add_scalar('loss_split/recons_loss', t['recons'].item(), epoch_num)
        self.writer.add_scalar('loss_split/dist_loss', (t['dist'] / self.beta).item(), epoch_num)
        if t['reg'] is not None:
            self.writer.add_scalar('loss_split/reg_loss', (t['reg'] / self.gamma).item(), epoch_num)

    # -- evaluation-only inference (measure_vae_trainer.py:188-212) ---------------------------------------------------
    def compute_representations(self, data_loader, num_batches=None):
        """-> (latent codes, attribute labels (n, 4), attribute names) over at most num_batches + 1 batches."""
        num_batches = 200 if num_batches is None else num_batches
        codes, attrs = [], []
        self.model.eval()
        with torch.no_grad():
            for i, batch in enumerate(data_loader):
                score, metadata = self.process_batch_data(batch)
                codes.append(self.model(score, metadata, train=False)[4])
                attrs.append(self.compute_attribute_labels(score))
                if i == num_batches:
                    break
        if not codes:
            raise ValueError('compute_representations: the loader produced no batch (split smaller than the batch size?)')
        return torch.cat(codes).cpu().numpy(), torch.cat(attrs).cpu().numpy(), list(self.attr_dict)

    def save_representations(self, path, data_loader=None, batch_size=256, num_batches=None):
        """Write the record the reference's compute_eval_metrics consumes (measure_vae_trainer.py:217-243): latent codes,
        attribute labels and attribute names as JSON, from the encoder-only pass.  compute_eval_metrics computes the
        disentanglement metrics from the same arrays (arvae_amd.evaluation); the reference's utils/evaluation.py also runs
        unchanged on this file's arrays."""
        import json
        if data_loader is None:
            _, _, data_loader = self.dataset.data_loaders(batch_size=batch_size)
        codes, attrs, names = self.compute_representations(data_loader, num_batches)
        with open(path, 'w') as f:
            json.dump({'latent_codes': codes.tolist(), 'attributes': attrs.tolist(), 'attr_list': list(names)}, f)
        return codes, attrs, names

    def compute_eval_metrics(self, batch_size=256, random_state=None):
        """results_dict.json next to the checkpoint, as in the reference (measure_vae_trainer.py:217-243): loaded when it exists,
        otherwise created on the device: the disentanglement metrics of the reference (interpretability, Corr_score,
        modularity_score, mig, SAP_score: arvae_amd.evaluation, its KSG estimator in HIP), the test loss / accuracy, and
        representations.json (the codes and attributes they were computed from).  Non-finite metric values are written as JSON
        null; an evaluation split of at most n_neighbors points leaves the metric keys out with a warning.  random_state: the
        KSG noise draws (None: fresh, as in the reference; an int s: the c-th KSG call uses RandomState(s + c))."""
        import json
        import os
        folder = os.path.dirname(self.model.filepath)
        results_fp = os.path.join(folder, 'results_dict.json')
        if os.path.exists(results_fp):
            with open(results_fp) as f:
                self.metrics = json.load(f)
            return self.metrics
        os.makedirs(folder, exist_ok=True)
        rep_fp = os.path.join(folder, 'representations.json')
        from .evaluation import eval_metrics_or_warn
        codes, attrs, names = self.save_representations(rep_fp, batch_size=batch_size)
        self.metrics = {'representations': rep_fp}
        self.metrics.update(eval_metrics_or_warn(codes, attrs, names, random_state=random_state))
        self.metrics.update(self.test_model(batch_size=batch_size))
        with open(results_fp, 'w') as f:
            json.dump(self.metrics, f, indent=2)
        return self.metrics

    def playable_mask(self, allowed=None):
        """uint8 (V,) flags of the notes a generated measure may hold: every entry of the dataset's index dictionaries except the
        padding symbols START, END and None (the slur '__' and 'rest' stay: they are music); an explicit `allowed` mask is
        intersected with it."""
        names = self.dataset.index2note_dicts
        v = len(names)
        mask = torch.tensor([0 if names[i] in _PADDING_SYMBOLS else 1 for i in range(v)], dtype=torch.uint8)
        if allowed is not None:
            mask = mask & self.model.decoder.sampling_filter(allowed=allowed)[2]
        return mask

    @staticmethod
    def _check_beam_draws_nothing(sampling, temperature, uniforms, top_k, top_p):
        if sampling == 'beam':
            given = [n for n, on in (('top_k', top_k is not None), ('top_p', top_p is not None), ('temperature', temperature != 1.0),
                                     ('uniforms', uniforms is not None)) if on]
            if given:
                raise ValueError(f"sampling='beam' draws nothing: {', '.join(given)} cannot be combined with it")

    def decode_latent_codes(self, latent_codes, sampling='argmax', temperature=1.0, uniforms=None, top_k=None, top_p=None, allowed=None,
                            playable=False, beam_width=4, plan=None):
        """(n, z_dim) latent codes -> (music21 score or None, note indices (n, 1, 24) int64): the decoder alone, free-running
        (measure_vae_trainer.py:281-288).  The score object needs the dataset's music21 converter (`tensor_to_m21score`);
        datasets without one (the device-resident loaders here) give None.  sampling='multinomial': every fed-back note is drawn
        from softmax(probs / temperature) (HierarchicalDecoder.generate; uniforms: explicit (n, 24) draws) instead of the top-1;
        top_k / top_p / allowed cut that draw (generate), playable=True keeps START, END and None out of it (playable_mask).
        sampling='beam': the most likely measure of every code among beam_width beams over the allowed / playable notes
        (HierarchicalDecoder.beam_search); nothing is drawn, so top_k, top_p, temperature and uniforms are refused with it.
        plan: a note plan (24, V) or (n, 24, V) (HierarchicalDecoder.note_plan; `build_note_plan`), honoured by all three modes and
        intersected with allowed / playable; with it 'argmax' takes the best allowed note."""
        dev = next(self.model.parameters()).device
        z = torch.as_tensor(latent_codes, dtype=torch.float32, device=dev).contiguous()
        self._check_beam_draws_nothing(sampling, temperature, uniforms, top_k, top_p)
        if playable:
            allowed = self.playable_mask(allowed)
        if sampling == 'beam':
            tensor_score = self.model.decoder.beam_search(z, beam_width=beam_width, allowed=allowed, plan=plan)[1]
            to_score = getattr(self.dataset, 'tensor_to_m21score', None)
            return (to_score(tensor_score) if callable(to_score) else None), tensor_score
        if sampling == 'argmax' and top_k is None and top_p is None and allowed is None and plan is None:
            dummy = torch.zeros(z.size(0), self.model.num_ticks_per_measure, dtype=torch.int64, device=dev)
            with torch.no_grad():
                _, tensor_score = self.model.decoder(z, dummy, False)
        else:
            _, tensor_score = self.model.decoder.generate(z, sampling=sampling, temperature=temperature, uniforms=uniforms, top_k=top_k,
                                                          top_p=top_p, allowed=allowed, plan=plan)
        to_score = getattr(self.dataset, 'tensor_to_m21score', None)
        return (to_score(tensor_score) if callable(to_score) else None), tensor_score

    def build_note_plan(self, score=None, keep=None, keep_rhythm=False, allowed=None, playable=False):
        """A note plan (n, 24, V) -- or (24, V) without a score -- for decode_latent_codes / infill_measures, as a bool CPU tensor.
        score (n, 24) or (n, 1, 24) note indices: the measures to keep parts of.  keep: bool (24,) or (n, 24), the ticks whose note of
        `score` is fixed (forced: that note is the only one allowed there).  keep_rhythm=True: a tick where `score` holds the slur
        '__' is forced to '__', and at every other tick '__' is banned, so onsets stay onsets.  allowed (V flags) / playable
        (playable_mask) apply at the free ticks only: a forced note stands even if it is not playable."""
        v, ticks = len(self.dataset.index2note_dicts), 24
        free = torch.ones(v, dtype=torch.bool)
        if playable:
            free = self.playable_mask(allowed) != 0
        elif allowed is not None:
            free = self.model.decoder.sampling_filter(allowed=allowed)[2] != 0
        if score is None:
            if keep is not None or keep_rhythm:
                raise ValueError('keep and keep_rhythm fix notes of a score: build_note_plan needs `score` with them')
            return free[None].expand(ticks, v).clone()
        notes = torch.as_tensor(score).detach().cpu()
        if notes.dim() == 3 and notes.shape[1] == 1:
            notes = notes[:, 0]
        if notes.dim() != 2 or notes.shape[1] != ticks or notes.dtype.is_floating_point:
            raise ValueError(f'score must hold note indices of shape (n, {ticks}) or (n, 1, {ticks}), got {tuple(torch.as_tensor(score).shape)}')
        notes = notes.to(torch.int64)
        if bool(((notes < 0) | (notes >= v)).any()):
            raise ValueError(f'score holds note indices outside [0, {v})')
        n = notes.shape[0]
        plan = free[None, None].expand(n, ticks, v).clone()
        forced = torch.zeros(n, ticks, dtype=torch.bool)
        if keep_rhythm:
            slur = self.dataset.note2index_dicts.get('__')
            if slur is None:
                raise ValueError("keep_rhythm needs the slur symbol '__' in the dataset's vocabulary")
            plan[:, :, slur] = False
            forced |= notes == slur
        if keep is not None:
            k = torch.as_tensor(keep).detach().cpu()
            if k.dtype != torch.bool or tuple(k.shape) not in ((ticks,), (n, ticks)):
                raise ValueError(f'keep must be a bool mask of shape ({ticks},) or ({n}, {ticks}), got {k.dtype} {tuple(k.shape)}')
            forced |= k.expand(n, ticks)
        one = torch.zeros(n, ticks, v, dtype=torch.bool).scatter_(2, notes[:, :, None], True)
        return torch.where(forced[:, :, None], one, plan)

    def infill_measures(self, score, keep=None, keep_rhythm=False, sampling='argmax', temperature=1.0, uniforms=None, top_k=None,
                        top_p=None, allowed=None, playable=False, beam_width=4):
        """Rewrite measures around what is kept of them: `score` (n, 24) / (n, 1, 24) is encoded to its posterior mean
        (encoder.encode_params) and decoded under build_note_plan(score, keep, keep_rhythm, allowed, playable) with sampling 'argmax',
        'multinomial' or 'beam' (decode_latent_codes).  The kept ticks come back as they were; the notes fed back into the decoder are
        the kept ones.  -> (music21 score or None, note indices (n, 1, 24) int64)"""
        if sampling not in ('argmax', 'multinomial', 'beam'):
            raise ValueError(f"sampling must be 'argmax', 'multinomial' or 'beam', got {sampling!r}")
        if keep is None and not keep_rhythm:
            raise ValueError('infill_measures keeps something of the score: give keep (the ticks to keep) or keep_rhythm=True')
        self._check_beam_draws_nothing(sampling, temperature, uniforms, top_k, top_p)
        plan = self.build_note_plan(score, keep, keep_rhythm, allowed, playable)
        if sampling != 'beam':                                 # (bad cuts are refused before the encoder runs)
            self.model.decoder.sampling_filter(top_k, top_p, None)
        dev = next(self.model.parameters()).device
        notes = torch.as_tensor(score).reshape(plan.shape[0], 24).to(device=dev, dtype=torch.int64).contiguous()
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                z = self.model.encoder.encode_params(notes)[0]
        finally:
            self.model.train(was_training)
        return self.decode_latent_codes(z, sampling=sampling, temperature=temperature, uniforms=uniforms, top_k=top_k, top_p=top_p,
                                        beam_width=beam_width, plan=plan)

    def decode_alternatives(self, latent_codes, beam_width, beam_groups, diversity, allowed=None, playable=False, plan=None):
        """(n, z_dim) latent codes -> (sequences (n, W, 24) int64, log_probs (n, W)): W = beam_width different likely measures per code
        by the diverse beam search (HierarchicalDecoder.beam_search with beam_groups / diversity), group-major and best first within
        a group, each with its log p(x | z) over the allowed notes.  allowed / playable / plan as decode_latent_codes."""
        dev = next(self.model.parameters()).device
        z = torch.as_tensor(latent_codes, dtype=torch.float32, device=dev).contiguous()
        if playable:
            allowed = self.playable_mask(allowed)
        res = self.model.decoder.beam_search(z, beam_width=beam_width, allowed=allowed, plan=plan, beam_groups=beam_groups,
                                             diversity=diversity)
        return res[3], res[5]

    def infill_alternatives(self, score, keep=None, keep_rhythm=False, allowed=None, playable=False, beam_width=4, beam_groups=2,
                            diversity=0.5):
        """Several ways to rewrite measures around what is kept of them: `score` is encoded to its posterior mean and decoded under
        build_note_plan(score, keep, keep_rhythm, allowed, playable) by decode_alternatives.  The kept ticks come back as they were in
        every alternative.  -> (sequences (n, W, 24) int64, log_probs (n, W))"""
        if keep is None and not keep_rhythm:
            raise ValueError('infill_alternatives keeps something of the score: give keep (the ticks to keep) or keep_rhythm=True')
        self.model.decoder.check_beam_groups(beam_width, beam_groups, diversity)      # refused before the encoder runs
        plan = self.build_note_plan(score, keep, keep_rhythm, allowed, playable)
        dev = next(self.model.parameters()).device
        notes = torch.as_tensor(score).reshape(plan.shape[0], 24).to(device=dev, dtype=torch.int64).contiguous()
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                z = self.model.encoder.encode_params(notes)[0]
        finally:
            self.model.train(was_training)
        return self.decode_alternatives(z, beam_width, beam_groups, diversity, plan=plan)

    def sample_measures(self, num, temperature=1.0, top_k=None, top_p=None, allowed=None, playable=False, beam_width=None):
        """num measures drawn from the model: z ~ N(0, I) from the library's generator, every note drawn from
        softmax(probs / temperature) over the notes top_k / top_p / allowed / playable leave (decode_latent_codes).
        beam_width W: the prior draws are decoded by beam search instead (sampling='beam'; no note is drawn).
        -> (music21 score or None, note indices (num, 1, 24) int64)"""
        dev = next(self.model.parameters()).device
        if beam_width is not None:
            mask = self.playable_mask(allowed) if playable else allowed
            self.model.decoder._beam_mask(beam_width, mask, 'cpu')   # a bad width or mask is refused before a draw is made
            if top_k is not None or top_p is not None or temperature != 1.0:
                raise ValueError("beam search draws no note: top_k, top_p and temperature cannot be combined with it")
            z = ops.normal_noise((int(num), self.model.latent_space_dim), dev)
            return self.decode_latent_codes(z, sampling='beam', beam_width=beam_width, allowed=mask)
        flt = (top_k, top_p, self.playable_mask(allowed) if playable else allowed)
        self.model.decoder.sampling_filter(*flt)                # bad cuts are refused before a draw is made
        z = ops.normal_noise((int(num), self.model.latent_space_dim), dev)
        return self.decode_latent_codes(z, sampling='multinomial', temperature=temperature, top_k=flt[0], top_p=flt[1], allowed=flt[2])

    def compute_latent_interpolations(self, latent_code, original_score=None, dim1=0, num_points=5):
        """Sweep latent dimension dim1 over [-4, 4] (measure_vae_trainer.py:290-308): all num_points codes are decoded in ONE
        batch instead of one decoder call per point.  -> (concatenated music21 score or None, note indices (num_points, 24))."""
        if num_points % 2 != 1:
            raise AssertionError('num_points must be odd')
        dev = next(self.model.parameters()).device
        z = torch.as_tensor(latent_code, dtype=torch.float32, device=dev).reshape(1, -1).repeat(num_points, 1)
        z[:, dim1] = torch.linspace(-4.0, 4.0, num_points, device=dev)
        scores, tensor_score = self.decode_latent_codes(z)
        tensor_score = tensor_score.squeeze(1)
        concat = getattr(self.dataset, 'concatenate_scores', None)
        to_score = getattr(self.dataset, 'tensor_to_m21score', None)
        score = None
        if callable(concat) and callable(to_score):
            parts = [to_score(tensor_score[i:i + 1, None, :]) for i in range(num_points)]
            if original_score is not None:
                parts[num_points // 2] = original_score
            score = concat(parts)
        return score, tensor_score

    # -- listening and looking: MIDI files and piano-roll PNGs (measure_vae_trainer.py:256-279, utils/plotting.py:307-362) ----------
    def _note_tables(self, device):
        """(build_measure_tables' tables, the slur's index): what ops.measure_notes / ops.render_pianoroll take"""
        slur = self.dataset.note2index_dicts.get('__')
        if slur is None:
            raise ValueError("the dataset's vocabulary has no slur symbol '__'")
        return self._attr_tables(device)[0], int(slur)

    def _look(self, look):
        """the reference's y-range of the dataset (utils/plotting.py:338-341) under the caller's look"""
        return {'pitch_lo': 55, 'pitch_hi': 90 if self.dataset_type == 'bach' else 84, **look}

    def write_measures(self, tensor_score, stem, values=None, attr_str=None, **look):
        """A sequence of measures -- note indices (K, 24), (K, 1, 24) or (24,) -- as <stem>.mid and <stem>.png: the note events and
        the piano roll come from one launch each (ops.measure_notes, ops.render_pianoroll) and reach the host in one copy each.
        values (K,): a number per measure, drawn as dots in a panel beside the roll; attr_str without values: that attribute's
        labels of the measures (compute_attribute_labels).  look: render_pianoroll's keywords.  -> (midi path, png path)"""
        import os
        from . import figures, midi
        dev = next(self.model.parameters()).device
        score = torch.as_tensor(tensor_score)
        score = score.reshape(-1, score.shape[-1]).to(device=dev, dtype=torch.int64).contiguous()
        tables, slur = self._note_tables(dev)
        events = ops.measure_notes(score, tables, slur=slur)
        if values is not None:
            values = torch.as_tensor(values, dtype=torch.float32).to(dev).reshape(1, score.shape[0])
        elif attr_str is not None:
            values = self.compute_attribute_labels(score, [attr_str]).reshape(1, score.shape[0])
        frame = ops.render_pianoroll(score[None], tables, values, slur=slur, **self._look(look))
        folder = os.path.dirname(stem)
        if folder:
            os.makedirs(folder, exist_ok=True)
        return midi.write_midi(stem + '.mid', events.cpu().numpy()), figures.write_png(frame, stem + '.png')

    def plot_latent_interpolations(self, latent_codes, attr_str, num_points=10, dim=None, sweep_points=5, **look):
        """For each of the first n = min(num_points, len(latent_codes)) codes: original_{i}.mid (the code decoded),
        latent_interpolations_{attr_str}_{i}.mid (the code with latent dimension `dim` swept over linspace(-4, 4, sweep_points), the
        middle measure replaced by the original) and latent_interpolations_{attr_str}_{i}.png (that sequence's piano roll with the
        attribute's value of each of its measures beside it) under Trainer.get_save_dir(model).  dim: by default the attribute's
        dimension of the interpretability metric (compute_eval_metrics).  All n * sweep_points + n codes are decoded in one batch,
        the labels come from one compute_attribute_labels call, the events from one launch and the n figures from one launch and
        one copy.  -> the paths written, per code in the order above"""
        import os
        from . import figures, midi
        if sweep_points % 2 != 1:
            raise AssertionError('sweep_points must be odd')
        if attr_str not in self.attr_dict:
            raise ValueError('Invalid regularization attribute')
        dev = next(self.model.parameters()).device
        codes = torch.as_tensor(latent_codes, dtype=torch.float32, device=dev)
        n = min(int(num_points), codes.shape[0])
        if n <= 0:
            return []
        if dim is None:
            metrics = self.metrics if 'interpretability' in self.metrics else self.compute_eval_metrics()
            if 'interpretability' not in metrics:
                raise RuntimeError('the figures sweep the dimension of the interpretability metric, which this evaluation split was '
                                   'too small to compute: give dim')
            dim = metrics['interpretability'][attr_str][0]
        p, codes = int(sweep_points), codes[:n]
        z = codes[:, None, :].repeat(1, p, 1)
        z[:, :, int(dim)] = torch.linspace(-4.0, 4.0, p, device=dev)
        tokens = self.decode_latent_codes(torch.cat([z.reshape(n * p, -1), codes]))[1].squeeze(1)
        t = tokens.shape[1]
        sweeps, originals = tokens[:n * p].reshape(n, p, t).clone(), tokens[n * p:]
        sweeps[:, p // 2] = originals
        labels = self.compute_attribute_labels(sweeps.reshape(n * p, t), [attr_str]).reshape(n, p)
        tables, slur = self._note_tables(dev)
        events = ops.measure_notes(torch.cat([sweeps.reshape(n * p, t), originals]), tables, slur=slur).cpu().numpy()
        frames = ops.render_pianoroll(sweeps, tables, labels.contiguous(), slur=slur, **self._look(look)).cpu().numpy()
        folder = Trainer.get_save_dir(self.model)
        paths = []
        for i in range(n):
            paths.append(midi.write_midi(os.path.join(folder, f'original_{i}.mid'), events[n * p + i:n * p + i + 1]))
            stem = os.path.join(folder, f'latent_interpolations_{attr_str}_{i}')
            paths.append(midi.write_midi(stem + '.mid', events[i * p:(i + 1) * p]))
            paths.append(figures.write_png(frames[i], stem + '.png'))
        return paths

    # -- the latent plane: where the data lies in it and what the decoder makes of it (measure_vae_trainer.py:245-254, 310-352,
    #    utils/plotting.py:41-63): scatter figures rendered on the device (ops.render_scatter), written by arvae_amd.figures ----------
    def plot_data_dist(self, latent_codes, attributes, attr_str, dim1=0, dim2=1, **look):
        """data_dist_{attr_str}.png under Trainer.get_save_dir(model): the codes in the plane (dim1, dim2), limits -4..4, coloured by
        the attribute's column of `attributes` (compute_representations' arrays).  attr_str may be a list of names, dim1 and dim2
        then one dimension for all or one a name: all figures come from one launch and one copy.  look: render_scatter's keywords.
        -> the path written (a list of paths for a list of names)"""
        from . import figures
        names = [attr_str] if isinstance(attr_str, str) else list(attr_str)
        for name in names:
            if name not in self.attr_dict:
                raise ValueError('Invalid regularization attribute')
        paths = figures.write_data_dist(self, latent_codes, attributes, names, [self.attr_dict[a] for a in names], dim1, dim2, look)
        return paths[0] if isinstance(attr_str, str) else paths

    def compute_latent_surface(self, dim1=0, dim2=1, grid_res=0.05, base_code=None, attr_list=None, chunk=4096):
        """The attributes of what the decoder makes of the plane (dim1, dim2): x = torch.arange(-5., 5., grid_res), n = len(x), code
        (i, j) of the grid holds x[i] in dimension dim1 and x[j] in dim2 (the reference's meshgrid) and base_code (z_dim,) elsewhere
        -- by default one standard-normal draw from the library's generator.  The n * n codes are decoded `chunk` at a time
        (decode_latent_codes, argmax) and labelled by compute_attribute_labels; every one of them is kept.
        -> (grid (n, n, 2), labels (n, n, A)) on the device, A = len(attr_list), by default all attributes"""
        dev = next(self.model.parameters()).device
        names = list(self.attr_dict) if attr_list is None else list(attr_list)
        if int(chunk) < 1:
            raise ValueError(f'chunk {chunk} must be positive')
        x = torch.arange(-5., 5., grid_res)
        z1, z2 = torch.meshgrid([x, x], indexing='ij')
        n = x.numel()
        if base_code is None:
            base = ops.normal_noise((1, self.model.latent_space_dim), dev)
        else:
            base = torch.as_tensor(base_code, dtype=torch.float32).reshape(1, -1).to(dev)
            if base.shape[1] != self.model.latent_space_dim:
                raise ValueError(f'base_code holds {base.shape[1]} numbers, a code {self.model.latent_space_dim}')
        grid = torch.stack([z1, z2], dim=2).to(dev)
        z = base.repeat(n * n, 1)
        z[:, int(dim1)], z[:, int(dim2)] = grid[:, :, 0].reshape(-1), grid[:, :, 1].reshape(-1)
        labels = []
        for at in range(0, n * n, int(chunk)):
            tokens = self.decode_latent_codes(z[at:at + int(chunk)])[1]
            labels.append(self.compute_attribute_labels(tokens.reshape(tokens.shape[0], -1), names))
        return grid, torch.cat(labels).reshape(n, n, len(names))

    def plot_latent_surface(self, attr_str, dim1=0, dim2=1, grid_res=0.05, base_code=None, **look):
        """latent_surface_{attr_str}.png under Trainer.get_save_dir(model): the grid of compute_latent_surface in the plane
        (dim1, dim2), limits -5..5, every code coloured by the attribute of the measure it decodes to.  attr_str may be a list of
        names: the grid is decoded once and all figures come from one launch and one copy; dim1 / dim2 may then hold one
        dimension a name, and every distinct plane is decoded once, around the same base code.  look: render_scatter's keywords.
        -> the path written (a list of paths for a list of names)"""
        import os
        from . import figures
        names = [attr_str] if isinstance(attr_str, str) else list(attr_str)
        for name in names:
            if name not in self.attr_dict:
                raise ValueError('Invalid regularization attribute')
        f = len(names)
        dims = [[int(d)] * f if np.ndim(d) == 0 else [int(x) for x in d] for d in (dim1, dim2)]
        if len(dims[0]) != f or len(dims[1]) != f:
            raise ValueError(f'plot_latent_surface: dim1 and dim2 are one dimension or {f} of them')
        if base_code is None:                                  # one draw for all planes
            base_code = ops.normal_noise((self.model.latent_space_dim,), next(self.model.parameters()).device)
        planes = sorted(set(zip(*dims)))                       # names that share a plane share its decode pass
        values = [None] * f
        for plane in planes:
            members = [i for i in range(f) if (dims[0][i], dims[1][i]) == plane]
            grid, labels = self.compute_latent_surface(plane[0], plane[1], grid_res, base_code, [names[i] for i in members])
            for k, i in enumerate(members):
                values[i] = labels[:, :, k].reshape(-1)
        n = grid.shape[0] * grid.shape[1]
        points = grid.reshape(1, n, 2).expand(f, n, 2).contiguous()          # (the grid is the same in every plane)
        look = {'labels': [(f'dimension: {a}', f'dimension: {b}') for a, b in zip(*dims)], **look}
        frames = ops.render_scatter(points, torch.stack(values).contiguous(), (-5.0, 5.0), (-5.0, 5.0), **look).cpu().numpy()
        folder = Trainer.get_save_dir(self.model)
        paths = [figures.write_png(frames[i], os.path.join(folder, f'latent_surface_{name}.png')) for i, name in enumerate(names)]
        return paths[0] if isinstance(attr_str, str) else paths

    def loss_and_acc_test(self, data_loader):
        """mean RECONSTRUCTION loss (no KL / regulariser terms) and mean top-1 accuracy over the loader's batches
        (measure_vae_trainer.py:367-397); accumulated on the device, one host sync at the end."""
        loss_sum = acc_sum = None
        count = 0
        with torch.no_grad():
            for batch in data_loader:
                score, metadata = self.process_batch_data(batch)
                fused = self.fused_executor(score)
                if fused is not None:                          # the executor's forward pass leaves both numbers in its scalars
                    from .fused_measure import ACC, RECON
                    enc = self.model.encoder
                    eps = enc._eps_queue.popleft() if enc._eps_queue else enc.static_eps
                    tables = fused.tables(self, score.device) if self.use_reg_loss else None
                    scalars = fused.run(score, False, None, tables, eps, None)[1]
                    loss, acc = scalars[RECON], scalars[ACC]
                else:
                    weights = self.model(measure_score_tensor=score, measure_metadata_tensor=metadata, train=False)[0]
                    loss, acc = ops.token_recon(weights, score)
                loss_sum = loss.detach().clone() if loss_sum is None else loss_sum + loss.detach()
                acc_sum = acc.detach().clone() if acc_sum is None else acc_sum + acc.detach()
                count += 1
        n = max(count, 1)
        return (float(loss_sum) / n if count else 0.0), (float(acc_sum) / n if count else 0.0)

    def test_model(self, batch_size):
        _, _, loader = self.dataset.data_loaders(batch_size)
        mean_loss, mean_acc = self.loss_and_acc_test(loader)
        print('Test Epoch:')
        print('\tTest Loss: ', mean_loss, '\n\tTest Accuracy: ', mean_acc * 100)
        return {'test_loss': mean_loss, 'test_acc': mean_acc}

    @staticmethod
    def reconstruction_loss(x, x_recons):
        return Trainer.mean_crossentropy_loss(weights=x_recons, targets=x)
