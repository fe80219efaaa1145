"""ImageVAETrainer: the AR-VAE loss step for the conv VAEs on the HIP kernels.

Loss recipe and API of the reference's imagevae/image_vae_trainer.py:65-217,
623-655:   loss = recon + beta*|KL - c| + sum_{d in reg_dim} gamma * reg(z[:,d], labels[:,d])
with the R-dimension Python loop replaced by one all-pairs kernel launch and the
two passes over the logits (BCE, accuracy) by one fused reduction.
"""
from typing import Tuple

import numpy as np
import os

import torch

from . import ops
from .trainer import Trainer

MNIST_REG_TYPES = {'digit_identity': 0, 'area': 1, 'length': 2, 'thickness': 3, 'slant': 4, 'width': 5,
                   'height': 6}
DSPRITES_REG_TYPE = {'color': 0, 'shape': 1, 'scale': 2, 'orientation': 3, 'posx': 4, 'posy': 5}
DATASET_REG_TYPE_DICT = {'mnist': MNIST_REG_TYPES, 'dsprites': DSPRITES_REG_TYPE}


def get_reg_dim(attr_dict):
    return tuple(v for k, v in attr_dict.items() if k not in ('digit_identity', 'color'))


class ImageVAETrainer(Trainer):
    def __init__(self, dataset, model, lr=1e-4, reg_type: Tuple[str] = None, reg_dim: Tuple[int] = 0,
                 dec_dist='bernoulli', beta=4.0, gamma=10.0, capacity=0.0, rand=0, delta=1.0):
        super().__init__(dataset, model, lr)
        kind = dataset.__class__.__name__
        if kind == 'MorphoMnistDataset':
            self.dataset_type = 'mnist'
        elif kind == 'DspritesDataset':
            self.dataset_type = 'dsprites'
        else:
            raise ValueError(f'Dataset type not recognized: {kind}')
        self.attr_dict = DATASET_REG_TYPE_DICT[self.dataset_type]
        self.reverse_attr_dict = {v: k for k, v in self.attr_dict.items()}
        self.metrics = {}
        self.beta = beta
        self.capacity = torch.tensor([capacity], dtype=torch.float32)
        self._capacity_nonzero = float(capacity) != 0.0
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
        self.dec_dist = dec_dist
        if len(self.reg_type) != 0:
            self.use_reg_loss = True
            self.reg_dim = reg_dim
            self.gamma = gamma
            self.delta = delta
            self.trainer_config += f'g_{self.gamma}_d_{self.delta}_' + '_'.join(self.reg_type) + '_'
        self.model.update_trainer_config(self.trainer_config)
        self.last_terms = {}
        self.use_fused = True          # whole-model C calls (arvae_amd.fused); False = one autograd node per layer
        self._fused = None
        # A TRAINING step (train=True, gradients enabled) leaves the forward pass's finishing step -- the sums that become the
        # loss, its split and the accuracy -- to the first launch of loss.backward() (ARVAE_VAE_DEFER_FINISH): those scalars are
        # final once backward() has run and read as NaN before.  The reference's loop (utils/trainer.py:136-147) and this
        # build's read them after step(); set False for code that looks at the loss between the two calls.
        self.defer_loss_finish = os.environ.get('ARVAE_DEFER_FINISH', '1') != '0'      # (the variable: same-box A/B runs)

    def cuda(self):
        super().cuda()
        self.capacity = self.capacity.cuda()

    def process_batch_data(self, batch):
        if self.dataset_type == 'mnist':
            inputs, _, labels = batch
        else:
            inputs, labels = batch
        dev = next(self.model.parameters()).device
        return (inputs.to(dev, torch.float32, non_blocking=True).contiguous(),
                labels.to(dev, torch.float32, non_blocking=True).contiguous())

    def loss_and_acc_for_batch(self, batch, epoch_num=None, batch_num=None, train=True):
        first_of_epoch = self.cur_epoch_num != epoch_num
        if first_of_epoch:
            self.cur_epoch_num = epoch_num
        inputs, labels = batch
        if self.capacity.device != inputs.device:
            self.capacity = self.capacity.to(inputs.device)
        if self.use_fused and inputs.is_cuda:
            return self._fused_loss_and_acc(inputs, labels, first_of_epoch, epoch_num, batch_num, train)

        outputs, z_dist, prior_dist, z_tilde, _ = self.model(inputs)
        recons_loss, accuracy = ops.image_recon(outputs, inputs, self.dec_dist)
        cap = self.capacity
        if self.data_parallel is not None and self._capacity_nonzero:   # |KL - c| needs the global KL mean (parallel.py)
            kl_local = self.compute_kld_loss(z_dist, prior_dist, beta=1.0, c=0.0).detach()
            cap = self.data_parallel.shifted_capacity(kl_local, self.capacity)
        dist_loss = self.compute_kld_loss(z_dist, prior_dist, beta=self.beta, c=cap)
        loss = recons_loss + dist_loss
        reg_loss = None
        if self.use_reg_loss:
            if type(self.reg_dim) != tuple:
                raise TypeError('Regularization dimension must be a tuple of integers')
            if self.data_parallel is not None:
                reg_loss = self.data_parallel.reg_loss(z_tilde, labels, self.reg_dim, self.gamma, self.delta)
            else:
                reg_loss = ops.reg_loss(z_tilde, labels, self.reg_dim, self.gamma, self.delta)
            loss = loss + reg_loss
        self.last_terms = {'recons': recons_loss.detach(), 'dist': dist_loss.detach(),
                           'reg': None if reg_loss is None else reg_loss.detach()}
        if first_of_epoch and self.writer is not None:
            self.writer.add_scalar('loss_split/recons_loss', recons_loss.item(), epoch_num)
            self.writer.add_scalar('loss_split/dist_loss', (dist_loss / self.beta).item(), epoch_num)
            if reg_loss is not None:
                self.writer.add_scalar('loss_split/reg_loss', (reg_loss / self.gamma).item(), epoch_num)
        if not train and batch_num == 0 and self.writer is not None:
            from .logging_utils import image_grid
            n = min(inputs.size(0), 16)
            self.writer.add_image('reconstruction',
                                  image_grid(torch.cat([inputs[:n], torch.sigmoid(outputs[:n].detach())]).cpu(), n),
                                  epoch_num)
        return loss, accuracy

    def _fused_loss_and_acc(self, inputs, labels, first_of_epoch, epoch_num, batch_num, train):
        """Same loss as above through arvae_image_vae_forward / _backward (one C call per pass)."""
        from .fused import DIST, RECON, REG, FusedImageVAE
        if type(self.reg_dim) != tuple and self.use_reg_loss:
            raise TypeError('Regularization dimension must be a tuple of integers')
        model = self.model
        if self._fused is None:
            self._fused = FusedImageVAE(model, self.optimizer, self.reg_dim if self.use_reg_loss else (), self.beta,
                                        self.gamma, self.delta, self.dec_dist)
        n = inputs.size(0)
        x = inputs.contiguous().view(n, model.image_hw, model.image_hw, 1)
        masks = model._next_masks(n, inputs.device)
        if model._eps_queue:                                     # explicit noise (parity runs)
            eps, draw = model._noise(torch.empty(n, model.z_dim, device=inputs.device)), False
        else:                                                    # drawn inside the fused heads kernel, written for backward
            eps, draw = torch.empty(n, model.z_dim, device=inputs.device), True
        dp = self.data_parallel
        # (the epoch's first batch is logged from the host right below: it finishes inside the forward pass)
        defer = train and self.defer_loss_finish and not (first_of_epoch and self.writer is not None)
        loss, scalars, accuracy, z, mu, sigma, logits = self._fused.run(x, labels, eps, masks, self.capacity, dp=dp,
                                                                       capacity_nonzero=self._capacity_nonzero, draw_eps=draw,
                                                                       defer_finish=defer)
        reg_loss = scalars[REG].detach() if self.use_reg_loss else None
        self.last_terms = {'recons': scalars[RECON].detach(), 'dist': scalars[DIST].detach(), 'reg': reg_loss}
        self.last_outputs = {'logits': logits.view(inputs.size()), 'z': z, 'mu': mu, 'sigma': sigma}
        if first_of_epoch and self.writer is not None:
            self.writer.add_scalar('loss_split/recons_loss', scalars[RECON].item(), epoch_num)
            self.writer.add_scalar('loss_split/dist_loss', scalars[DIST].item() / self.beta, epoch_num)
            if reg_loss is not None:
                self.writer.add_scalar('loss_split/reg_loss', reg_loss.item() / self.gamma, epoch_num)
        if not train and batch_num == 0 and self.writer is not None:
            from .logging_utils import image_grid
            k = min(n, 16)
            recon = torch.sigmoid(logits.view(inputs.size())[:k].detach())
            self.writer.add_image('reconstruction', image_grid(torch.cat([inputs[:k], recon]).cpu(), k), epoch_num)
        return loss, accuracy

    # -- evaluation-only inference (image_vae_trainer.py:264-288,381-403): encoder / decoder passes on the forward
    #    kernels; the metrics fed from here (utils/evaluation.py) are arvae_amd.evaluation's ---------------------------
    def _extract_relevant_attributes(self, attributes):
        attr_list = [a for a in self.attr_dict if a not in ('digit_identity', 'color')]
        return attributes[:, [self.attr_dict[a] for a in attr_list]], attr_list

    def compute_representations(self, data_loader, num_batches=200):
        """-> (latent codes (n, z_dim), attribute columns (n, k), attribute names); stops after num_batches + 1 batches
        like the reference (`if sample_id == 200: break` comes after the append)."""
        codes, attrs = [], []
        self.model.eval()
        with torch.no_grad():
            for i, batch in enumerate(data_loader):
                inputs, labels = self.process_batch_data(batch)
                codes.append(self.model(inputs)[3])
                attrs.append(labels)
                if i == num_batches:
                    break
        codes = torch.cat(codes).cpu().numpy()             # one device->host copy for the whole sweep
        attrs, names = self._extract_relevant_attributes(torch.cat(attrs).cpu().numpy())
        return codes, attrs, names

    def compute_latent_interpolations(self, latent_code, dim1=0, num_points=10):
        """Decoder sweep of one latent dimension over [-4, 4]: (num_points, 1, H, W) probabilities on the device."""
        dev = next(self.model.parameters()).device
        z = torch.as_tensor(latent_code, dtype=torch.float32, device=dev).reshape(1, -1).repeat(num_points, 1)
        z[:, dim1] = torch.linspace(-4.0, 4.0, num_points, device=dev)
        with torch.no_grad():
            return torch.sigmoid(self.model.decode(z.contiguous()))

    def compute_latent_interpolations2d(self, latent_code, dim1=0, dim2=1, num_points=10):
        dev = next(self.model.parameters()).device
        x = torch.linspace(-4.0, 4.0, num_points, device=dev)
        z1, z2 = torch.meshgrid([x, x], indexing='ij')
        z = torch.as_tensor(latent_code, dtype=torch.float32, device=dev).reshape(1, -1).repeat(num_points * num_points, 1)
        z[:, dim1], z[:, dim2] = z1.reshape(-1), z2.reshape(-1)
        with torch.no_grad():
            return torch.sigmoid(self.model.decode(z.contiguous()))

    # -- figures (image_vae_trainer.py:405-552): decoder logits -> file bytes in one render launch per figure
    #    (ops.render_frames: sigmoid, make_grid and the cast to uint8), written by arvae_amd.figures.  Every method returns the
    #    paths it wrote.  deterministic=True decodes the posterior mean instead of the sampled code: reproducible figures -----
    def _interpretability(self):
        """{attribute: (latent dimension, score)} of the evaluation metrics (results_dict.json, or computed now)"""
        if 'interpretability' not in self.metrics:
            self.compute_eval_metrics()
        if 'interpretability' not in self.metrics:
            raise RuntimeError('the figures sweep the dimensions of the interpretability metric, which this evaluation split was '
                               'too small to compute')
        return self.metrics['interpretability']

    def _eval_batch(self, number, batch_size=1):
        """(inputs, labels) of the number-th evaluation batch, without touching the batches before it; None past the end"""
        import itertools
        loader = self.dataset.data_loaders(batch_size=batch_size)[2]
        if hasattr(loader, 'batch_at'):
            batch = loader.batch_at(number)
        else:
            batch = next(itertools.islice(iter(loader), number, None), None)
        if batch is None:
            print(f'evaluation batch {number} (batch size {batch_size}) is past the end of the split: no figure')
            return None
        return self.process_batch_data(batch)

    def _code_and_logits(self, inputs, deterministic):
        """(z (B, z_dim), reconstruction logits (B, 1, H, W)): the forward pass's sampled code, or the posterior mean"""
        self.model.eval()
        with torch.no_grad():
            if deterministic:
                z = self.model.encode(inputs).loc
                return z, self.model.decode(z.contiguous())
            out = self.model(inputs)
            return out[3], out[0]

    def _decode_sweeps(self, z, sweeps):
        """logits of ONE decoder batch: for every entry of `sweeps`, a {latent dimension: values (P,)}, the code z (1, z_dim)
        repeated P times with those dimensions overwritten; the entries follow one another in the batch"""
        parts = []
        for sweep in sweeps:
            zs = z.repeat(next(iter(sweep.values())).numel(), 1)
            for d, values in sweep.items():
                zs[:, d] = values
            parts.append(zs)
        with torch.no_grad():
            return self.model.decode(torch.cat(parts).contiguous())

    def _save_dir(self):
        return Trainer.get_save_dir(self.model)

    def _write_original_and_recons(self, sample_id, inputs, recons_logits, rounding):
        from . import figures
        paths = []
        for name, src, logits in (('original', inputs, False), ('recons', recons_logits.view(inputs.size()), True)):
            frame = ops.render_frames(src.contiguous(), [[0]], nrow=1, pad_value=1.0, logits=logits, rounding=rounding)
            paths.append(figures.write_png(frame, os.path.join(self._save_dir(), f'{name}_{sample_id}.png')))
        return paths

    def create_latent_gifs(self, sample_id=9, num_points=10, deterministic=False):
        """gif_interpolations_{dataset_type}_{sample_id}.gif: num_points frames; frame n shows, side by side, the sample decoded
        with each attribute's latent dimension (attr_dict order) set to linspace(-4, 4, num_points)[n].  All attributes' sweeps
        leave the decoder as one batch."""
        from . import figures
        interp = self._interpretability()
        dims = [int(interp[a][0]) for a in self.attr_dict if a not in ('digit_identity', 'color')]
        batch = self._eval_batch(sample_id)
        if batch is None:
            return []
        z, _ = self._code_and_logits(batch[0], deterministic)
        sweep = torch.linspace(-4.0, 4.0, num_points, device=z.device)
        logits = self._decode_sweeps(z, [{d: sweep} for d in dims])                    # attribute-major: image a * num_points + n
        cells = np.arange(len(dims) * num_points).reshape(len(dims), num_points).T     # cells[n][a] = a * num_points + n
        frames = ops.render_frames(logits, cells, nrow=8, padding=2, pad_value=1.0, logits=True, rounding=False)
        path = os.path.join(self._save_dir(), f'gif_interpolations_{self.dataset_type}_{sample_id}.gif')
        return [figures.write_gif(frames, path)]

    def plot_latent_interpolations(self, attr_str='slant', num_points=10, sample_ids=(5, 1, 30, 19, 23, 21, 17, 61, 9, 28),
                                   deterministic=False, rounding=True):
        """per sample: latent_interpolations_{attr_str}_{id}.png (one row: the attribute's dimension over linspace(-4, 4,
        num_points)), original_{id}.png and recons_{id}.png.  Samples past the end of the evaluation split are left out, as in the
        reference's loop."""
        from . import figures
        dim = int(self._interpretability()[attr_str][0])
        paths = []
        for sample_id in sample_ids:
            batch = self._eval_batch(sample_id)
            if batch is None:
                continue
            z, recons = self._code_and_logits(batch[0], deterministic)
            logits = self._decode_sweeps(z, [{dim: torch.linspace(-4.0, 4.0, num_points, device=z.device)}])
            frame = ops.render_frames(logits, [list(range(num_points))], nrow=num_points, pad_value=1.0, rounding=rounding)
            paths.append(figures.write_png(frame, os.path.join(self._save_dir(), f'latent_interpolations_{attr_str}_{sample_id}.png')))
            paths += self._write_original_and_recons(sample_id, batch[0], recons, rounding)
        return paths

    def plot_latent_interpolations2d(self, attr_str1, attr_str2, num_points=10, sample_id=9, deterministic=False, rounding=True):
        """latent_interpolations_2d_({attr_str1},{attr_str2})_{id}.png: the num_points x num_points grid of
        compute_latent_interpolations2d ('ij': attr_str1's dimension changes down the rows, attr_str2's along them), with
        original_{id}.png and recons_{id}.png"""
        from . import figures
        interp = self._interpretability()
        dim1, dim2 = int(interp[attr_str1][0]), int(interp[attr_str2][0])
        batch = self._eval_batch(sample_id)
        if batch is None:
            return []
        z, recons = self._code_and_logits(batch[0], deterministic)
        x = torch.linspace(-4.0, 4.0, num_points, device=z.device)
        z1, z2 = torch.meshgrid([x, x], indexing='ij')
        logits = self._decode_sweeps(z, [{dim1: z1.reshape(-1), dim2: z2.reshape(-1)}])
        frame = ops.render_frames(logits, [list(range(num_points * num_points))], nrow=num_points, pad_value=1.0, rounding=rounding)
        path = os.path.join(self._save_dir(), f'latent_interpolations_2d_({attr_str1},{attr_str2})_{sample_id}.png')
        return [figures.write_png(frame, path)] + self._write_original_and_recons(sample_id, batch[0], recons, rounding)

    def plot_latent_reconstructions(self, num_points=10, deterministic=False, rounding=True):
        """r_original_0.png / r_recons_0.png: the first evaluation batch of num_points images and its reconstructions, one row each"""
        from . import figures
        batch = self._eval_batch(0, batch_size=num_points)
        if batch is None:
            return []
        inputs = batch[0]
        _, recons = self._code_and_logits(inputs, deterministic)
        cells = [list(range(inputs.size(0)))]
        paths = []
        for name, src, logits in (('r_original_0', inputs, False), ('r_recons_0', recons.view(inputs.size()), True)):
            frame = ops.render_frames(src.contiguous(), cells, nrow=num_points, pad_value=1.0, logits=logits, rounding=rounding)
            paths.append(figures.write_png(frame, os.path.join(self._save_dir(), f'{name}.png')))
        return paths

    def plot_data_dist(self, latent_codes, attributes, attr_str, dim1=0, dim2=1, **look):
        """data_dist_{attr_str}.png under Trainer.get_save_dir(model) (image_vae_trainer.py:370-379): the codes in the plane
        (dim1, dim2), limits -4..4, coloured by the attribute, as a scatter figure rendered on the device (ops.render_scatter).
        attributes: compute_representations' columns (the attributes without digit_identity / color, in attr_dict's order) or all
        of the dataset's label columns (indexed by attr_dict).  attr_str may be a list of names, dim1 and dim2 then one dimension
        for all or one a name: all figures come from one launch and one copy.  look: render_scatter's keywords.
        -> the path written (a list of paths for a list of names)"""
        from . import figures
        names = [attr_str] if isinstance(attr_str, str) else list(attr_str)
        relevant = [a for a in self.attr_dict if a not in ('digit_identity', 'color')]
        width = np.shape(attributes)[1]
        if width == len(relevant) and width != len(self.attr_dict):
            column = {a: i for i, a in enumerate(relevant)}
        elif width > max(self.attr_dict.values()):
            column = dict(self.attr_dict)
        else:
            raise ValueError(f'attributes holds {width} columns: neither the {len(relevant)} of compute_representations nor the labels')
        for name in names:
            if name not in column:
                raise ValueError('Invalid regularization attribute')
        paths = figures.write_data_dist(self, latent_codes, attributes, names, [column[a] for a in names], dim1, dim2, look)
        return paths[0] if isinstance(attr_str, str) else paths

    def save_representations(self, path, data_loader=None, batch_size=128):
        """Write the record the reference's compute_eval_metrics consumes (image_vae_trainer.py:289-317): latent codes,
        attribute columns and attribute names as JSON, from the encoder-only pass.  compute_eval_metrics computes the
        disentanglement metrics from the same arrays (arvae_amd.evaluation); the reference's utils/evaluation.py also runs
        unchanged on this file's arrays."""
        import json
        if data_loader is None:
            _, _, data_loader = self.dataset.data_loaders(batch_size=batch_size)
        codes, attrs, names = self.compute_representations(data_loader)
        with open(path, 'w') as f:
            json.dump({'latent_codes': codes.tolist(), 'attributes': np.asarray(attrs).tolist(), 'attr_list': list(names)}, f)
        return codes, attrs, names

    def compute_eval_metrics(self, batch_size=128, random_state=None):
        """results_dict.json next to the checkpoint, as in the reference (image_vae_trainer.py:289-317): loaded when it exists,
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
        if self.dataset_type == 'mnist' and 'interpretability' in self.metrics:
            from .mnist_resnet import MnistResNet
            if os.path.exists(MnistResNet().filepath):     # (the reference fails without the classifier; here the key is left out)
                self.metrics.update(self.get_resnet_accuracy(batch_size=batch_size))
        with open(results_fp, 'w') as f:
            json.dump(self.metrics, f, indent=2)
        return self.metrics

    def get_resnet_accuracy(self, batch_size=128, resnet_model=None, record=None):
        """{'digit_pred_acc': {'inputs', 'recons', 'interp'}} of the reference (image_vae_trainer.py:319-368): the share of the
        evaluation digits that the ResNet-18 classifier (arvae_amd.mnist_resnet, HIP) recognises as given, after reconstruction,
        and after each latent dimension of self.metrics['interpretability'] has been swept over linspace(-4, 4, 10) in the
        decoder (z.repeat(10, 1) with that dimension overwritten; labels digit_labels.repeat(10)).  Each figure is the mean over
        the batches of per-batch accuracies; 'interp' is also averaged over the keys.
        The reference's quirk is kept, so that the number compares with its own: the keys include the metric's 'mean' entry
        (-1, m), i.e. the LAST latent dimension is swept as a seventh "attribute" and the divisor is 7, not 6.
        None unless the dataset is Morpho-MNIST.  resnet_model None: MnistResNet() loaded from its checkpoint.  record: a list
        that receives (kind, images, labels, predictions) for every classified batch, kind in 'inputs' | 'recons' | 'interp:<key>'.
        Accuracies accumulate on the device: one host sync at the end."""
        if self.dataset_type != 'mnist':
            return None
        dev = next(self.model.parameters()).device
        if resnet_model is None:
            from .mnist_resnet import MnistResNet
            resnet_model = MnistResNet()
            if not os.path.exists(resnet_model.filepath):
                raise FileNotFoundError(
                    f'{resnet_model.filepath}: the digit classifier\'s checkpoint is missing; the reference publishes it as '
                    'MnistRESNET.pt (its README, "Downloading Models"): put it there or set ARVAE_MODEL_DIR')
            resnet_model.load(cpu=True)
            resnet_model.to(dev)
        if 'interpretability' not in self.metrics:
            self.compute_eval_metrics(batch_size=batch_size)
        if 'interpretability' not in self.metrics:
            raise RuntimeError('digit_pred_acc sweeps the dimensions of the interpretability metric, which this evaluation split '
                               'was too small to compute')
        interp_dict = self.metrics['interpretability']
        _, _, loader = self.dataset.data_loaders(batch_size=batch_size)
        num_interps = 10
        sums = torch.zeros(3, device=dev)
        count = 0
        self.model.eval()

        def accuracy(kind, images, labels):
            pred = self.compute_mnist_digit_identity(resnet_model, images)
            if record is not None:
                record.append((kind, images, labels, pred))
            return self.mean_accuracy_pred(pred, labels)

        with torch.no_grad():
            for batch in loader:
                inputs, digit_labels = batch[0], batch[1]
                inputs = inputs.to(dev, torch.float32).contiguous()
                digit_labels = digit_labels.to(dev, torch.int64)
                out = self.model(inputs)
                recons, z = torch.sigmoid(out[0]), out[3]
                sums[0] += accuracy('inputs', inputs, digit_labels)
                sums[1] += accuracy('recons', recons.view(inputs.shape), digit_labels)
                b = z.size(0)
                z_rep = z.repeat(num_interps, 1)
                sweep = torch.linspace(-4.0, 4.0, num_interps, device=dev).repeat_interleave(b)
                labels_rep = digit_labels.repeat(num_interps)
                per_key = torch.zeros((), device=dev)
                for key, entry in interp_dict.items():
                    z_copy = z_rep.clone()
                    z_copy[:, int(entry[0])] = sweep
                    outputs = torch.sigmoid(self.model.decode(z_copy.contiguous())).view(num_interps * b, 1, 28, 28)
                    per_key += accuracy(f'interp:{key}', outputs, labels_rep)
                sums[2] += per_key / len(interp_dict)
                count += 1
        inputs_acc, recons_acc, interp_acc = (sums / max(count, 1)).tolist()
        return {'digit_pred_acc': {'inputs': inputs_acc, 'recons': recons_acc, 'interp': interp_acc}}

    def loss_and_acc_test(self, data_loader):
        """mean RECONSTRUCTION loss (no KL / regulariser terms) and mean pixel accuracy over the loader's batches
        (image_vae_trainer.py:595-621); accumulated on the device, one host sync at the end."""
        loss_sum = acc_sum = None
        count = 0
        with torch.no_grad():
            for batch in data_loader:
                inputs, _ = self.process_batch_data(batch)
                outputs = self.model(inputs)[0]
                loss, acc = ops.image_recon(outputs, inputs, self.dec_dist)
                loss_sum = loss.detach().clone() if loss_sum is None else loss_sum + loss.detach()
                acc_sum = acc.detach().clone() if acc_sum is None else acc_sum + acc.detach()
                count += 1
        n = max(count, 1)
        return (float(loss_sum) / n if count else 0.0), (float(acc_sum) / n if count else 0.0)

    def test_model(self, batch_size):
        """Mean reconstruction loss / accuracy over the evaluation split (image_vae_trainer.py:582-593)."""
        _, _, loader = self.dataset.data_loaders(batch_size)
        mean_loss, mean_acc = self.loss_and_acc_test(loader)
        print('Test Epoch:')
        print('\tTest Loss: ', mean_loss, '\n\tTest Accuracy: ', mean_acc * 100)
        return {'test_loss': mean_loss, 'test_acc': mean_acc}

    # -- static helpers (image_vae_trainer.py:623-655) ---------------------------------------------------
    @staticmethod
    def reconstruction_loss(x, x_recons, dist):
        if dist not in ('bernoulli', 'gaussian'):
            raise AttributeError('invalid dist')
        return ops.image_recon(x_recons, x, dist)[0]

    @staticmethod
    def mean_accuracy_pred(pred_labels, gt_labels):
        """share of equal labels, a device scalar (image_vae_trainer.py:657-660)"""
        return (pred_labels.long() == gt_labels.long()).float().mean()

    @staticmethod
    def compute_mnist_digit_identity(resnet_model, outputs):
        """argmax labels (int64, on the device) of the classifier in evaluation mode (image_vae_trainer.py:662-666); MnistResNet
        returns the head kernel's argmax, any other module's probabilities go through torch.max"""
        resnet_model.eval()
        with torch.no_grad():
            if hasattr(resnet_model, 'predict'):
                return resnet_model.predict(outputs)
            return torch.max(resnet_model(outputs), 1)[1]

    @staticmethod
    def mean_accuracy(weights, targets):
        """weights are probabilities (sigmoid already applied by the caller, as in the reference)."""
        logits = torch.logit(weights.detach().clamp(0.0, 1.0))     # p >= .5  <=>  logit >= 0
        return ops.image_recon(logits.nan_to_num(posinf=1e30, neginf=-1e30), targets, 'bernoulli')[1]
