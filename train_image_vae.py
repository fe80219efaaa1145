#!/usr/bin/env python3
"""Train / evaluate the image AR-VAEs on MI355X: counterpart of the reference's train_image_vae.py (same flags and
defaults, same `models/<repr>/<repr>.pt` and `runs/` side effects, same reg_type -> reg_dim mapping and seed loop).

Differences a user can observe: the dataset lives in HBM (arvae_amd.data), a single `-r <name>` works (the
reference indexes its attribute table with the whole tuple there and raises KeyError), `--no_log` survives the
second epoch, and after training the script prints a representation summary computed on the device (latent codes /
attributes of the evaluation split, test loss and accuracy); `--metrics` adds the reference's disentanglement metrics
(Interpretability, SCC, Modularity, MIG, SAP: arvae_amd.evaluation, KSG estimator in HIP) to it, and `--digit_acc` (Morpho-MNIST
only) the reference's digit_pred_acc: the accuracy of the ResNet-18 digit classifier (arvae_amd.mnist_resnet, HIP) on the
inputs, the reconstructions and the latent sweeps; it needs the classifier's checkpoint, models/MnistRESNET/MnistRESNET.pt.
`--gifs` writes the reference's latent-traversal GIFs (create_latent_gifs for samples 0, 1 and 4) and `--plots` the PNG figures of
its commented-out block (plot_latent_reconstructions, plot_latent_interpolations per attribute, plot_latent_interpolations2d)
into models/<repr>/results/, rendered on the device (arvae_amd.ops.render_frames, HIP).  `--data_dist` writes data_dist_<attr>.png
there for every attribute (plot_data_dist: the test codes in the plane of the attribute's dimension and a free one, a scatter figure
rendered on the device, arvae_amd.ops.render_scatter).
"""
import json
import os
import sys

import click
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from arvae_amd.evaluation import eval_metrics_or_warn  # noqa: E402
from arvae_amd.data import DspritesDataset, MorphoMnistDataset  # noqa: E402
from arvae_amd.image_vae import DspritesVAE, MnistVAE  # noqa: E402
from arvae_amd.image_vae_trainer import DSPRITES_REG_TYPE, MNIST_REG_TYPES, ImageVAETrainer  # noqa: E402


def reg_dims_for(reg_type, attr_dict, skip=('digit_identity', 'color')):
    """The reference's --reg_type -> latent dimension mapping (train_image_vae.py:72-91)."""
    if len(reg_type) == 0:
        return (0,)
    if len(reg_type) == 1 and reg_type[0] == 'all':
        return tuple(v for k, v in attr_dict.items() if k not in skip)
    return tuple(attr_dict[r] for r in reg_type)


# flag surface of the reference script (names, defaults and help strings are the drop-in contract), kept as a table
IMAGE_FLAGS = [
    (('--dataset_type', '-d'), dict(default='mnist', help='dataset to be used, `mnist` or `dsprites`')),
    (('--batch_size',), dict(default=128, help='training batch size')),
    (('--num_epochs',), dict(default=100, help='number of training epochs')),
    (('--lr',), dict(default=1e-4, help='learning rate')),
    (('--beta',), dict(default=4.0, help='parameter for weighting KLD loss')),
    (('--capacity',), dict(default=0.0, help='parameter for beta-VAE capacity')),
    (('--gamma',), dict(default=10.0, help='parameter for weighting regularization loss')),
    (('--delta',), dict(default=1.0, help='parameter for controlling the spread')),
    (('--dec_dist',), dict(default='bernoulli', help='distribution of the decoder')),
    (('--train/--test',), dict(default=True, help='train or test the specified model')),
    (('--log/--no_log',), dict(default=False, help='log the results for tensorboard')),
    (('--rand',), dict(default=None, help='random seed for the random number generator')),
    (('--reg_type', '-r'), dict(default=None, multiple=True, help='attribute name string to be used for regularization')),
]
# not in the reference script (whose evaluation always prints the metrics): opt-in here, so that the summary stays as it was.  It
# is read by run() around the reference's flag surface (main's parameters stay exactly the reference's)
METRICS_FLAG = '--metrics'
METRICS_HELP = (f'{METRICS_FLAG}: add the disentanglement metrics (Interpretability, SCC, Modularity, MIG, SAP; '
                'arvae_amd.evaluation) to the evaluation summary.')
with_metrics = False
DIGIT_ACC_FLAG = '--digit_acc'
DIGIT_ACC_HELP = (f'{DIGIT_ACC_FLAG}: (mnist only) add digit_pred_acc, the ResNet-18 digit classifier\'s accuracy on inputs, '
                  'reconstructions and latent sweeps, to the evaluation summary; needs models/MnistRESNET/MnistRESNET.pt.')
with_digit_acc = False
GIFS_FLAG = '--gifs'
GIFS_HELP = (f'{GIFS_FLAG}: write the latent-traversal GIFs of evaluation samples 0, 1 and 4 (create_latent_gifs) into '
             'models/<repr>/results/.')
with_gifs = False
PLOTS_FLAG = '--plots'
PLOTS_HELP = (f'{PLOTS_FLAG}: write the PNG figures (reconstructions, the latent interpolations of every attribute, the 2-d grid '
              'of slant / thickness for mnist, posx / posy for dsprites) into models/<repr>/results/.')
with_plots = False
DATA_DIST_FLAG = '--data_dist'
DATA_DIST_HELP = (f'{DATA_DIST_FLAG}: for every attribute write data_dist_{{attr}}.png into models/<repr>/results/, the codes of the '
                  'test split (batches of 128, at most 100 of them) in the plane of the attribute\'s dimension of the interpretability '
                  'metric and the last dimension that belongs to no attribute, coloured by the attribute (plot_data_dist).')
with_data_dist = False


def with_options(fn):
    for names, kwargs in reversed(IMAGE_FLAGS):
        fn = click.option(*names, **kwargs)(fn)
    return click.command(epilog='\n\n'.join((METRICS_HELP, DIGIT_ACC_HELP, GIFS_HELP, PLOTS_HELP, DATA_DIST_HELP)))(fn)


def write_data_dist(trainer, dataset, metrics, batch_size):
    """plot_data_dist for every attribute the interpretability metric names, as the reference's music script does it
    (train_measure_vae.py:188-197): batches of 128 of the test split, at most 100 of them; -> the paths written"""
    interp = metrics['interpretability']
    attr_names = [a for a in trainer.attr_dict if a in interp]
    attr_dims = [int(interp[a][0]) for a in attr_names]
    other = [d for d in range(trainer.model.z_dim) if d not in attr_dims][-1]
    _, _, loader = dataset.data_loaders(batch_size=min(128, batch_size))
    codes, attrs, _ = trainer.compute_representations(loader, num_batches=min(100, len(loader)))
    return trainer.plot_data_dist(codes, attrs, attr_names, attr_dims, other)


def write_figures(trainer, dataset_type, gifs, plots):
    """the reference script's figure calls (train_image_vae.py:127-153); -> the paths written"""
    paths = []
    if gifs:
        for sample_id in (0, 1, 4):
            paths += trainer.create_latent_gifs(sample_id=sample_id)
    if plots:
        paths += trainer.plot_latent_reconstructions()
        for attr_str in trainer.attr_dict:
            if attr_str not in ('digit_identity', 'color'):
                paths += trainer.plot_latent_interpolations(attr_str)
        paths += trainer.plot_latent_interpolations2d(*(('slant', 'thickness') if dataset_type == 'mnist' else ('posx', 'posy')))
    return paths


@with_options
def main(dataset_type, batch_size, num_epochs, lr, beta, capacity, gamma, delta, dec_dist, train, log, rand, reg_type):
    if dataset_type == 'mnist':
        dataset, attr_dict = MorphoMnistDataset(), MNIST_REG_TYPES
    elif dataset_type == 'dsprites':
        dataset, attr_dict = DspritesDataset(), DSPRITES_REG_TYPE
    else:
        raise ValueError('Invalid dataset_type. Choose between mnist and dsprites')
    reg_dim = reg_dims_for(reg_type, attr_dict)
    seeds = range(0, 10) if rand is None else [int(rand)]
    # launched by torch.distributed.run: one process per GPU, minibatch rows sharded over the ranks, gradients all-reduced
    # over RCCL (arvae_amd.parallel); --batch_size is then the per-GPU batch
    from arvae_amd.parallel import init_from_env
    dp = init_from_env() if train else None
    chief = dp is None or dp.rank == 0

    def build(seed):
        # the reference builds the model BEFORE the trainer seeds torch (train_image_vae.py:97-109, image_vae_trainer.py:103):
        # its initial weights differ from run to run.  Here the run's seed covers them too (same run, same weights)
        torch.manual_seed(seed)
        model = MnistVAE() if dataset_type == 'mnist' else DspritesVAE()
        trainer = ImageVAETrainer(dataset=dataset, model=model, lr=lr, reg_type=reg_type, reg_dim=reg_dim, beta=beta,
                                  capacity=capacity, gamma=gamma, delta=delta, dec_dist=dec_dist, rand=seed)
        return model, trainer

    # every rank trains every seed first; rank 0 evaluates afterwards, once the process group is gone -- a rank that waits in
    # a pending RCCL collective while rank 0 evaluates would be killed by the group's watchdog timeout (advisor, round 2)
    if train:
        if not torch.cuda.is_available():
            raise SystemExit('training needs a GPU: the AR-VAE path has no CPU fallback')
        try:
            for seed in seeds:
                model, trainer = build(seed)
                trainer.cuda()
                if dp is not None:
                    dp.attach(trainer)
                trainer.train_model(batch_size=batch_size, num_epochs=num_epochs, log=log)
                trainer.data_parallel = None
            if dp is not None:
                dp.finish()
        except BaseException:
            # a rank that fails must not leave its peers waiting in a collective: give the communicator up without waiting for
            # them (ncclCommAbort) and let the error end this process non-zero -- the launcher then ends the other ranks, whose
            # own bounded waits (parallel.LibraryComm.wait_idle) raise in the meantime
            if dp is not None:
                dp.abort()
            raise
    if not chief:
        return
    for seed in seeds:
        model, trainer = build(seed)
        trainer.load_model()
        trainer.writer = None
        eval_bs = min(128, batch_size)                  # the reference evaluates with 128; smaller runs keep their own size
        _, _, eval_loader = dataset.data_loaders(batch_size=eval_bs)
        codes, attrs, names = trainer.compute_representations(eval_loader)
        summary = {'model': repr(model), 'num_codes': int(codes.shape[0]), 'attributes': names,
                   'latent_mean_abs': [float(v) for v in abs(codes).mean(0)]}
        summary.update(trainer.test_model(batch_size=eval_bs))
        want_figures = with_gifs or with_plots or with_data_dist
        metrics = eval_metrics_or_warn(codes, attrs, names) if with_metrics or want_figures or (with_digit_acc and dataset_type == 'mnist') else {}
        if with_metrics:
            summary.update(metrics)
        if with_digit_acc and dataset_type != 'mnist':
            print(f'{DIGIT_ACC_FLAG}: the digit classifier applies to mnist only; skipped for {dataset_type}')
        elif with_digit_acc:
            trainer.metrics = dict(metrics)              # the sweeps run over the interpretability metric's dimensions
            summary.update(trainer.get_resnet_accuracy(batch_size=eval_bs))
        print(json.dumps(summary, indent=2))
        if want_figures and 'interpretability' not in metrics:
            print(f'{GIFS_FLAG} / {PLOTS_FLAG} / {DATA_DIST_FLAG}: the figures use the dimensions of the interpretability metric, which this '
                  f'evaluation split ({codes.shape[0]} codes) was too small to compute; skipped')
        elif want_figures:
            trainer.metrics = dict(metrics)
            for path in write_figures(trainer, dataset_type, with_gifs, with_plots):
                print('wrote', path)
            if with_data_dist:
                trainer.cuda()
                for path in write_data_dist(trainer, dataset, metrics, batch_size):
                    print('wrote', path)


def run(argv=None):
    """the command line: the reference's flags (main) plus this build's opt-in --metrics, --digit_acc, --gifs, --plots and --data_dist"""
    global with_metrics, with_digit_acc, with_gifs, with_plots, with_data_dist
    argv = sys.argv[1:] if argv is None else list(argv)
    with_metrics = METRICS_FLAG in argv
    with_digit_acc = DIGIT_ACC_FLAG in argv
    with_gifs = GIFS_FLAG in argv
    with_plots = PLOTS_FLAG in argv
    with_data_dist = DATA_DIST_FLAG in argv
    main(args=[a for a in argv if a not in (METRICS_FLAG, DIGIT_ACC_FLAG, GIFS_FLAG, PLOTS_FLAG, DATA_DIST_FLAG)])


if __name__ == '__main__':
    run()
