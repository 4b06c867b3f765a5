#!/usr/bin/env python
"""Drop-in for the reference's ``python main.py --model <name> --mode train|overfit|predict`` (main.py:22-373)
on the MI355X-native hot path.

Same flags (including the inverted ``--recon`` store_false, main.py:32), same ``experiments/<model>/params.json``
keys, same registry shape ``name -> (ModelCls, loss_fn, predict_fn, metric)`` (main.py:258-265), same step loop
(main.py:55-80, metrics every ``--eval_every`` epochs) and the same artefacts: checkpoints in
``model_dir + str(train_frac)`` like main.py:188, ``losses_tr.npy`` / ``losses_ev.npy`` / ``metrics_tr.npy`` /
``metrics_ev.npy`` in model_dir.  New, optional:
  --synthetic N     train on N synthetic GTSRB/GTSDB-shaped samples (the reference ships no data)
  --n_epochs E, --batch_size B   override params.json
  --fix_ckpt_dir    save checkpoints into model_dir, where --restore looks for them
  --clip_norm X, --skip_nonfinite   global gradient-norm clipping and a guard against non-finite steps, both decided on the device
                    inside capsyolo_amd.optim.Adam (params.json keys clip_norm, skip_nonfinite)
  --ema D [--ema_warmup]   an exponential moving average of the parameters with decay D in (0, 1), kept inside capsyolo_amd.optim.Adam's
                    launch (params.json keys ema_decay, ema_warmup): every evaluation of the training loop, hence
                    eval metric, `best` and best.pth.tar, judges the averaged weights, and the checkpoints gain 'ema_state_dict' (the
                    averages under the model's parameter names) next to 'state_dict' and 'optim_dict', which stay what they were.
                    --ema_warmup: d_t = min(D, (1 + t) / (10 + t)).  Buffers (BatchNorm running statistics) are not averaged.
                    best.pth.tar's 'state_dict' holds the LIVE weights of the epoch whose AVERAGED weights scored best: `--restore best`
                    without --use_ema runs weights that were not the ones judged.
  --use_ema         --mode predict | detect | serve | interpret: run on the checkpoint's 'ema_state_dict' (detector, and the --combine
                    classifier when its checkpoint has one); a checkpoint written without --ema is refused
  params.json keys ``n_iter`` (routing iterations, default 3), ``sync_bn`` (data parallel only)
  --model darkcapsule2 | darkcapsule3   the reference's unwired variants with their losses (models.py:271-337, 403-463)
``--mode predict --model darknet_d|darknet_r --combine cnn|capsule --restore last|best`` runs the two-stage chain
(predict_fns.dark_class_pred) and writes detect_and_recog_mAP / detect_and_recog_acc to combine-<name>_metric_output.txt
(main.py:329-356); ``--mode predict --model cnn|capsule --restore last|best`` runs the classifier over the test set and writes
recog_pr / recog_acc / recog_auc to metric_output.txt (main.py:309-317, 349-356), the curves counted on the device
(metrics.recog_report).  ``--draw`` (new) makes the combined branch write its annotated images to <model_dir>/output/<i>.ppm.
``--mode detect --model darknet_d|darknet_r --restore last|best [--synthetic N]`` is the reference's detect-only predict branch
(main.py:319-327, 349-363: `--mode predict` without `--combine` there).  It is a mode of its own here because `--mode predict`
without `--combine` has always exited with a message for the detectors, and callers rely on that.  It writes detect_AP /
detect_acc to metric_output.txt and the images with the predictions in green and the ground truth in red, drawn on the device, to
<model_dir>/output/<i>.ppm (see detect()).  The metric curves are not plotted.
``--mode serve --model darknet_d|darknet_r --combine cnn|capsule --restore last|best [--synthetic N] [--graph] [--max_boxes K]``
(new) restores both checkpoints once and pushes the test frames one at a time through the streaming detector
(capsyolo_amd.serve.SignDetector: frame in, labelled boxes out, nothing crosses to the host between the two networks; ``--graph``
replays a captured HIP graph per frame shape).  It writes one line per frame to <model_dir>/serve_output.txt and prints the
latency percentiles (see serve()).
``--nms IOU [--nms_class_aware]`` (new; with --mode detect, --mode predict --combine and --mode serve) runs greedy non-maximum
suppression over the detector's boxes on the device (`cy_nms_boxes`) before they are cropped, drawn or scored: the metric files
then hold the metrics of the suppressed predictions, and one line says how many boxes over 0.5 the step removed.  The reference
has no such step, so the default is none.  ``--per_frame N`` (serve only) keeps at most the N most confident survivors of a frame.
``--tiles RxC --tile_overlap PX [--tile_full] [--tile_margin M]`` (new; with --mode serve and --mode detect, both with --nms, and with
--mode train --model darknet_d|darknet_r --augment) runs the detector on R x C overlapping windows of every frame at close to native
scale instead of on the resized frame (capsyolo_amd.tiles): the windows' boxes are put back into the frame on the device
(`cy_yolo_decode_tiles_conf`), the duplicates in the overlaps are merged by the suppression step, and the outputs keep their
formats; in train mode every augmented sample is one randomly drawn window with the labels of the signs visible in it.
``--mode serve ... --track [--max_tracks N --track_iou X --max_misses M --min_hits H --track_decay D --no_motion]`` (new) follows the
boxes from frame to frame on the device (`cy_track_update` behind serve.SignTracker): track ids, classes voted over a track's frames,
hit counts; one line per frame goes to <model_dir>/tracks_output.txt, serve_output.txt stays as it is.
``--mode serve ... --frame_format nv12 [--yuv_matrix NAME] [--device_frames]`` (new) hands the detector NV12 frames (encoded from the
RGB frames with capsyolo_amd.nv12.from_rgb), converted inside the two crop launches; ``--device_frames`` (either format) uploads each
frame before the timed call and passes a device tensor.
``--mode interpret --model capsule --restore last|best [--synthetic N] [--index I]`` is the reference's capsule_interpret.py:
the 16 x 11 perturbation sweep of sample I's labelled capsule through the fused decoder kernel, written to <model_dir>/img/
(see interpret()).
``--mode attack --model capsule|cnn --restore last|best [--use_ema] [--synthetic N] --eps 0,1,2,4,8 [--attack fgsm|pgd --attack_steps K
--attack_alpha A] [--index I]`` (new) measures the restored classifier's accuracy under a bounded perturbation of every test image
(capsyolo_amd.attack: the gradient with respect to the image on the project's kernels; ``--eps`` and ``--attack_alpha`` in grey levels) and
writes one ``eps:accuracy, `` entry per level to <model_dir>/attack_output.txt; with ``--index`` also sample I clean, perturbed at the
largest level, and its saliency map as attack_<I>_clean.ppm / _adv.ppm / _saliency.ppm (see attack()).  ``--model cnn`` needs
``--cnn_kernels hip``.
``--mode train --model darknet_d|darknet_r|darkcapsule* --augment [--gtsrb DIR] [--synthetic N]`` (new) trains on the reference's
sign-paste augmentation (build_data.py:171-288) made fresh for every batch on the device instead of frozen as ``--aug N`` copies:
the raw frames of <data_dir>/train_raw.p (``build_data.py --keep_raw``) stay on the device, ``add_signs`` comes from params.json
(default 0), the eval set is not augmented (see augmented_data()).
``--mode train|overfit --model cnn|capsule --class_augment [--synthetic N] [--graph]`` (new) trains the classifiers on the reference's
shift-and-lightness augmentation (utils.py:126-143, `utils.augmentation`, dead code there) drawn fresh per sample and per epoch: the
training set stays on the device as bytes and every batch is one gather kernel (capsyolo_amd.class_augment).  Optional params.json
keys ``aug_max_shift`` (pixels, default 4) and ``aug_max_light`` (on the 0..1 V scale, default 0.05); both 0 give the resident feed
without jitter.  The eval set is not augmented (see class_augmented_data()).  ``--augment`` stays the detectors' flag.
``--model cnn --cnn_kernels hip`` (new; also for the ``--combine cnn`` classifier; params.json key ``cnn_kernels``, default ``torch``) runs
ConvNet on the project's kernels with its Adam and ``--graph`` instead of nn.Conv2d / nn.Linear / torch.optim.Adam; it needs a GPU.
Data-parallel: launch with ``python -m torch.distributed.run --nproc-per-node N main.py ...``; every rank takes
its equal shard of each global batch, gradients are averaged with one RCCL all-reduce per step, epoch losses are
averaged over the ranks before the LR scheduler sees them, metrics run on the gathered predictions, rank 0 writes.
tensorboardX and torchsummary are outside the hot path; the registry's metrics (main.py:259-264) run through
capsyolo_amd.metrics (detection metrics on the device), ``--no_metric`` skips them like the reference.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import capsyolo_amd  # noqa: E402,F401
from capsyolo_amd import augment, class_augment, config, dp, metrics, synth, utils  # noqa: E402
from capsyolo_amd import interpret as capsule_interpret  # noqa: E402
from capsyolo_amd.input_pipeline import DeviceFeeder, quantize_if_exact  # noqa: E402
from capsyolo_amd.loss_fns import (capsule_loss, cnn_loss, dark_loss, darkcapsule2_loss, darkcapsule3_loss,  # noqa: E402
                                   darkcapsule_loss)
from capsyolo_amd.models import CapsuleNet, ConvNet, DarkCapsuleNet, DarkCapsuleNet2, DarkCapsuleNet3, DarkNet  # noqa: E402
from capsyolo_amd.optim import Adam  # noqa: E402
from capsyolo_amd.predict_fns import class_pred, class_scores_device, dark_class_pred, dark_forward, dark_pred  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument('--model', default='cnn', help=' | '.join(config.model_names))
parser.add_argument('--mode', default='train', help='train | predict | detect | serve | overfit | interpret | attack')
parser.add_argument('--summary', default=True, help='if summarize model', action='store_true')
parser.add_argument('--seed', type=int, default=0, help='random seed')
parser.add_argument('--lr', type=float, default=1e-3, help='learning rate')
parser.add_argument('--dropout', type=float, default=-1, help='dropout rate')
parser.add_argument('--train_frac', type=float, default=1, help='fraction of train data')
parser.add_argument('--restore', default=None, help="last | best")
parser.add_argument('--combine', default=None, help="cnn | capsule: the classifier behind --model darknet_d|darknet_r in predict mode")
parser.add_argument('--draw', default=False, action='store_true',
                    help='--mode predict --combine: also write the images with the boxes drawn to <model_dir>/output/<i>.ppm')
parser.add_argument('--recon', help='if use reconstruction loss', action='store_false')
parser.add_argument('--recon_coef', default=5e-4, help='reconstruction coefficient')
parser.add_argument('--eval_every', default=1, type=int, help='evaluate metric every # epochs')
parser.add_argument('--fine_tune', default=-1, type=int, help='number of fixed layer in fine tuning')
parser.add_argument('--no_metric', help='do not compute metric', action='store_true')
parser.add_argument('--model_dir', default=None, help='model dir')
parser.add_argument('--show', default=False, help='save result', action='store_true')
parser.add_argument('--npy', default=False, help='data is npy file', action='store_true')
parser.add_argument('--synthetic', type=int, default=0, help='use N synthetic samples instead of data/')
class _StoreGiven(argparse.Action):
    """store, and note in <dest>_given that the option was on the command line (a default cannot tell)."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + '_given', True)


parser.add_argument('--index', type=int, default=0, action=_StoreGiven,
                    help='--mode interpret: which sample of the eval set (or of the --synthetic samples).  --mode attack: when given, '
                         'also write this test sample clean, perturbed and as a saliency map')
parser.set_defaults(index_given=False)
parser.add_argument('--eps', default=None, metavar='E0,E1,...',
                    help='--mode attack: the perturbation bounds in grey levels (1 = 1/128 of the centred input), e.g. 0,1,2,4,8')
parser.add_argument('--attack', default='fgsm', choices=('fgsm', 'pgd'), help='--mode attack: one signed-gradient step, or projected steps')
parser.add_argument('--attack_steps', type=int, default=10, metavar='K', help='--attack pgd: number of steps')
parser.add_argument('--attack_alpha', type=float, default=None, metavar='A',
                    help='--attack pgd: step size in grey levels (default: 2.5 * eps / steps)')
parser.add_argument('--n_epochs', type=int, default=0, help='override params.json n_epochs')
parser.add_argument('--batch_size', type=int, default=0, help='override params.json batch_size')
parser.add_argument('--graph', action='store_true',
                    help='capture the training step (forward + loss + backward + Adam) once in a HIP graph and replay it per batch: '
                         'for the launch-bound small models (capsule); single process only.  --mode serve: capture the '
                         'detector -> classifier chain once per frame shape')
parser.add_argument('--augment', action='store_true',
                    help='--mode train of a detector: paste GTSRB signs over the raw frames on the device, fresh for every batch')
parser.add_argument('--class_augment', action='store_true',
                    help='--mode train|overfit of a classifier (cnn | capsule): shift and lightness jitter per sample and epoch, '
                         'made on the device from the resident training set')
parser.add_argument('--cnn_kernels', default=None, choices=('torch', 'hip'),
                    help='--model cnn and the --combine cnn classifier: override params.json cnn_kernels (torch: nn.Conv2d / nn.Linear; '
                         'hip: the conv blocks and the linear kernels of this project, with its Adam; needs a GPU)')
parser.add_argument('--gtsrb', default=config.GTSRB, help='--augment: the GTSRB root whose Images/ are the signs to paste')
parser.add_argument('--max_boxes', type=int, default=16,
                    help='--mode serve: box slots per call (the classifier always runs on this many crops; further boxes are dropped)')
parser.add_argument('--nms', type=float, default=None, metavar='IOU',
                    help='--mode detect | predict --combine | serve: non-maximum suppression of the detector\'s boxes at this IoU '
                         '(in [0, 1]) before crops, drawing and metrics; default: none')
parser.add_argument('--nms_class_aware', action='store_true',
                    help='--nms: a box is suppressed only by a box of the same detector class (a detector with class scores: darknet_r)')
parser.add_argument('--per_frame', type=int, default=0, metavar='N',
                    help='--mode serve --nms: at most N boxes of a frame survive, the most confident ones (0: no cap)')
parser.add_argument('--tiles', default=None, metavar='RxC',
                    help='--mode serve | detect (with --nms), --mode train --augment: run the detector on R x C overlapping windows of '
                         'a frame at close to native scale instead of on the resized frame (capsyolo_amd.tiles)')
parser.add_argument('--tile_overlap', type=int, default=None, metavar='PX',
                    help='--tiles: neighbouring windows overlap by at least PX pixels (more than the largest sign; default 0)')
parser.add_argument('--tile_full', action='store_true', help='--tiles: the whole frame is one more view (for signs larger than the overlap)')
parser.add_argument('--tile_margin', type=float, default=None, metavar='M',
                    help='--tiles: a box within M tile pixels of a window edge inside the frame is left to the neighbouring window '
                         '(default 2; negative: keep all)')
parser.add_argument('--track', action='store_true',
                    help='--mode serve: join the boxes of successive frames into tracks on the device (ids, voted classes, hit counts); '
                         'one line per frame goes to <model_dir>/tracks_output.txt')
parser.add_argument('--max_tracks', type=int, default=None, metavar='N', help='--track: track slots (default 32, at most 256)')
parser.add_argument('--track_iou', type=float, default=None, metavar='X',
                    help='--track: a box joins a track at an IoU above this with its predicted box (default 0.3)')
parser.add_argument('--max_misses', type=int, default=None, metavar='M',
                    help='--track: a track ends after more than M frames in a row without a box (default 2)')
parser.add_argument('--min_hits', type=int, default=None, metavar='H', help='--track: a track is reported as confirmed from H boxes on (default 2)')
parser.add_argument('--track_decay', type=float, default=None, metavar='D',
                    help='--track: weight in [0, 1] of the older class scores in a track\'s class vote (default 0.9)')
parser.add_argument('--no_motion', action='store_true', help='--track: match against a track\'s last box, not against the box moved on by its last step')
parser.add_argument('--frame_format', default='rgb', choices=['rgb', 'nv12'],
                    help='--mode serve: what the detector is handed.  nv12: every frame is encoded to NV12 first (capsyolo_amd.nv12.from_rgb, '
                         'odd frames lose their last row / column) and read in place by the two crop launches')
parser.add_argument('--yuv_matrix', default=None, metavar='NAME',
                    help='--frame_format nv12: the coefficient row, one of bt601 (default), bt709, bt601_full, bt709_full')
parser.add_argument('--device_frames', action='store_true',
                    help='--mode serve: the frames are uploaded before the timed call and handed over as device tensors')
parser.add_argument('--clip_norm', type=float, default=None, metavar='X',
                    help='clip the global gradient norm of every step to X (params.json key clip_norm): inside the project\'s Adam on the '
                         'device, without rewriting the gradients; torch.nn.utils.clip_grad_norm_ for the plain-torch cnn baseline')
parser.add_argument('--skip_nonfinite', action='store_true',
                    help='a step with an inf or NaN gradient leaves parameters and optimizer state as they are, decided on the device '
                         '(params.json key skip_nonfinite); needs the project\'s Adam')
parser.add_argument('--ema', type=float, default=None, metavar='D',
                    help='keep an exponential moving average of the parameters with decay D in (0, 1) inside the project\'s Adam launch '
                         '(params.json key ema_decay); evaluation, best and the checkpoint\'s ema_state_dict use the averaged weights. '
                         'best.pth.tar is then chosen by the averaged weights\' metric while its state_dict holds the live ones: restore it '
                         'with --use_ema to run what was judged')
parser.add_argument('--ema_warmup', action='store_true',
                    help='--ema: decay min(D, (1 + t) / (10 + t)) at a parameter\'s step t (params.json key ema_warmup)')
parser.add_argument('--use_ema', action='store_true',
                    help='--mode predict | detect | serve | interpret: load the checkpoint\'s ema_state_dict into the model\'s parameters')
parser.add_argument('--fix_ckpt_dir', action='store_true',
                    help='save checkpoints into model_dir (where --restore reads) instead of model_dir + str(train_frac)')

model_loss_predict = {
    'cnn': (ConvNet, cnn_loss, class_pred, metrics.recog_acc),                    # main.py:259-260
    'capsule': (CapsuleNet, capsule_loss, class_pred, metrics.recog_acc),
    'darknet_d': (DarkNet, dark_loss, dark_forward, metrics.detect_acc),          # main.py:261; on the device here
    'darknet_r': (DarkNet, dark_loss, dark_forward, metrics.detect_and_recog_acc),        # main.py:262
    'darkcapsule': (DarkCapsuleNet, darkcapsule_loss, None, metrics.detect_and_recog_acc),   # main.py:264 (the later key wins)
    # the reference's unwired variants with their own losses (models.py:271-337, 403-463; loss_fns.py:145-184)
    'darkcapsule2': (DarkCapsuleNet2, darkcapsule2_loss, None, None),
    'darkcapsule3': (DarkCapsuleNet3, darkcapsule3_loss, None, None),
}
# what predict mode reports for detector + classifier (main.py:342-346): name -> metric(y, y_hat, params), in this order
combine_metrics = {'detect_and_recog_mAP': metrics.detect_and_recog_mAP,          # sets params.n_classes = 43 (metrics.py:285)
                   'detect_and_recog_acc': metrics.detect_and_recog_acc}


def _batches(x, y, batch_size):
    n_batch = (len(y) + batch_size - 1) // batch_size
    return n_batch, zip(np.array_split(x, n_batch), np.array_split(y, n_batch))        # main.py:45-47


_warned = set()


def _shard(x_bch, y_bch, params):
    """This rank's contiguous, EQUAL shard of a global batch.  np.array_split makes near-equal batches (600 / 32 ->
    11 x 32 + 8 x 31, main.py:47); equal shards are what makes the mean of the ranks' gradients the global-batch
    gradient (each loss divides by its local batch), so up to world-1 samples of a batch that does not divide are left
    out, with one warning."""
    rank, world = params.rank, params.world
    if world > 1:
        per = len(y_bch) // world
        if len(y_bch) % world and 'rem' not in _warned and rank == 0:
            _warned.add('rem')
            print('data parallel: batches of %d samples on %d ranks: %d sample(s) per such batch are not used'
                  % (len(y_bch), world, len(y_bch) % world), flush=True)
        x_bch, y_bch = x_bch[rank * per:(rank + 1) * per], y_bch[rank * per:(rank + 1) * per]
    return x_bch, y_bch


def _feed(it, params, source=None):
    """main.py:57-59 (H2D + float + NHWC->NCHW) through the buffered device-side pipeline; batches smaller than
    the number of ranks are dropped on every rank alike.  source (--augment, training only): the batches are frame numbers, and
    the samples are made on the device by its feeder."""
    shards = [_shard(x_np, y_np, params) for x_np, y_np in it]
    shards = [(x_np, y_np) for x_np, y_np in shards if len(y_np) > 0]
    if source is not None:
        return source.feeder([x_np for x_np, _ in shards])
    if params.device == 'cpu':          # only the plain-torch `cnn` baseline gets here (main() refuses the others)
        return _host_batches(shards)
    return DeviceFeeder(shards, params.device)


def _host_batches(shards):
    """main.py:57-59 as written, for the plain-torch baseline model on a machine without a GPU."""
    for x_np, y_np in shards:
        if x_np.dtype == np.uint8:      # quantize_if_exact() stored the centred set as bytes
            x_np = (x_np.astype(np.float32) - 128.0) * np.float32(0.0078125)
        yield torch.from_numpy(x_np).float().permute(0, 3, 1, 2).contiguous(), torch.from_numpy(y_np)


def _forward(model, loss_fn, x_bch, y_bch, params):
    if params.model == 'capsule' and params.recon:                                       # main.py:61-66
        y_hat, recon = model(x_bch, y_bch, True)
        return y_hat, loss_fn(y_hat, y_bch, params, x_bch, recon)
    y_hat = model(x_bch)
    return y_hat, loss_fn(y_hat, y_bch, params)


def _gather(t, params):
    """Concatenate a per-rank tensor over the ranks (equal shards) -- metrics are computed on the global predictions."""
    if params.world == 1:
        return t
    import torch.distributed as dist
    parts = [torch.empty_like(t) for _ in range(params.world)]
    dist.all_gather(parts, t.contiguous())
    return torch.cat(parts)


def _metric(metric, y_true, y_hat, params):
    """main.py:82-91 / 129-137: the metric on at most config.max_metric_samples samples drawn like the reference does
    (np.random.choice with replacement, only when there are more samples than that)."""
    if metric is None or not y_hat:
        return -1
    y_true, y_hat = _gather(torch.cat(y_true), params), _gather(torch.cat(y_hat), params)
    n, cap = y_true.shape[0], getattr(config, 'max_metric_samples', 1000)
    if n > cap:
        idx = torch.from_numpy(np.random.choice(n, cap).astype(np.int64)).to(y_true.device)
        y_true, y_hat = y_true[idx], y_hat[idx]
    try:
        return float(metric(y_true, y_hat, params))
    except ValueError as e:     # e.g. darkcapsule's [B,g,g,5] output has no class scores for its registry metric
        if params.rank == 0:    # (the reference stops here, metrics.py:267-268; pass --no_metric to skip the attempt)
            print('metric not computed: %s' % e)
        return -1


def _mean_over_ranks(value, params):
    """Epoch losses are per-rank means over equal shards: their mean over the ranks is the global epoch loss.  Every rank
    must see the SAME number (ReduceLROnPlateau steps on it: a rank-local loss would let the replicas' learning rates
    drift apart)."""
    if params.world == 1:
        return value
    import torch.distributed as dist
    t = torch.tensor([value], dtype=torch.float64, device=params.device if dist.get_backend() == 'nccl' else 'cpu')
    dist.all_reduce(t)
    return float(t.item()) / params.world


def train(x, y, model, optimizer, loss_fn, metric, params, bucket, if_eval=True):
    """main.py:42-95.  The step loop keeps the predictions on the device (no per-step D2H copy: the reference's
    y_hat.append(... .cpu().numpy()), main.py:68, exists only to feed the metric below) and reads the loss value once
    per step like the reference's progress bar does (main.py:74-77)."""
    model.train()
    x, y = utils.shuffle(x, y)
    n_batch, it = _batches(x, y, params.batch_size)
    avg_loss, avg_iou, y_hat, y_true = 0.0, 0.0, [], []
    # --skip_nonfinite: the epoch loss is the mean over the steps with a finite loss value (a skipped batch would hand NaN to
    # ReduceLROnPlateau); the value is read every step anyway
    guard, finite_sum, finite_n = getattr(params, 'skip_nonfinite', False), 0.0, 0
    clip_torch = getattr(params, 'clip_norm', None) if not isinstance(optimizer, Adam) else None
    want_metric = if_eval and metric is not None
    graphed = getattr(params, 'graph', False) and params.world == 1 and params.device != 'cpu'
    for x_bch, y_bch in _feed(it, params, getattr(params, 'augment_source', None)):
        if graphed:
            # the whole step as one graph replay (capsyolo_amd/graph_step.py); captured on the first batch of this shape
            key = (id(model), id(optimizer), tuple(x_bch.shape), tuple(y_bch.shape))
            steps = params.__dict__.setdefault('_graph_steps', {})
            if key not in steps:                          # (one capture per batch shape: the ragged last batch gets its own)
                from capsyolo_amd.graph_step import GraphedStep
                steps[key] = GraphedStep(model, lambda m, xb, yb: _forward(m, loss_fn, xb, yb, params), optimizer, (x_bch, y_bch))
            y_hat_bch, loss = steps[key](x_bch, y_bch)
            if want_metric:
                y_hat.append(y_hat_bch.detach().clone())  # the graph's output tensor is overwritten by the next replay
                y_true.append(y_bch.detach().clone())
            value = loss.item()
            if not guard:
                avg_loss += value / n_batch
            elif np.isfinite(value):
                finite_sum, finite_n = finite_sum + value, finite_n + 1
            if params.model == 'darknet_d':
                avg_iou += params.avg_iou.item() / n_batch
            continue
        y_hat_bch, loss = _forward(model, loss_fn, x_bch, y_bch, params)
        if want_metric:
            y_hat.append(y_hat_bch.detach())
            y_true.append(y_bch.detach().clone())        # the feeder's slot buffers are overwritten by later batches
        optimizer.zero_grad()
        loss.backward()
        bucket.allreduce_mean()
        if clip_torch is not None:                       # the plain-torch cnn baseline; optim.Adam clips inside its step
            torch.nn.utils.clip_grad_norm_([p for g in optimizer.param_groups for p in g['params']], clip_torch)
        optimizer.step()
        value = loss.item()
        if not guard:
            avg_loss += value / n_batch
        elif np.isfinite(value):
            finite_sum, finite_n = finite_sum + value, finite_n + 1
        if params.model == 'darknet_d':
            avg_iou += params.avg_iou.item() / n_batch
    if guard:
        avg_loss = finite_sum / finite_n if finite_n else float('nan')
    score = _metric(metric, y_true, y_hat, params) if want_metric else -1
    if params.model == 'darknet_d' and params.rank == 0:
        print('train avg iou: {:05.3f}'.format(avg_iou), flush=True)
    return avg_loss, score


def evaluate(x, y, model, loss_fn, metric, params, if_eval=True):
    """main.py:98-143."""
    model.eval()
    n_batch, it = _batches(x, y, params.batch_size)
    avg_loss, y_hat, y_true = 0.0, [], []
    want_metric = if_eval and metric is not None
    with torch.no_grad():
        for x_bch, y_bch in _feed(it, params):
            y_hat_bch, loss = _forward(model, loss_fn, x_bch, y_bch, params)
            avg_loss += loss.item() / n_batch
            if want_metric:
                y_hat.append(y_hat_bch.detach().clone())
                y_true.append(y_bch.detach().clone())
    return avg_loss, (_metric(metric, y_true, y_hat, params) if want_metric else -1)


def checkpoint_dir(model_dir, params):
    """The reference saves checkpoints to model_dir + str(train_frac) (e.g. experiments/darkcapsule1, main.py:188) but
    restores from model_dir (main.py:149).  Same here by default; --fix_ckpt_dir saves where --restore reads."""
    return model_dir if getattr(params, 'fix_ckpt_dir', False) else model_dir + str(params.train_frac)


def train_and_evaluate(model, optimizer, loss_fn, metric, params, data, model_dir, restore_file=None):
    """main.py:146-217."""
    if restore_file is not None:
        utils.load_checkpoint(os.path.join(model_dir, restore_file + '.pth.tar'), model, params, optimizer)
    x_tr, y_tr, x_ev, y_ev = data
    to_frac = int(y_tr.shape[0] * params.train_frac)
    x_tr, y_tr = x_tr[:to_frac], y_tr[:to_frac]
    # centred images that are exactly (uint8 - 128) / 128 are kept as bytes (once per data set): 4-8x less to shuffle
    # and to move over PCIe, converted back on the device (input_pipeline.py)
    x_tr, x_ev = [q if q is not None else x for q, x in ((quantize_if_exact(x), x) for x in (x_tr, x_ev))]
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, 'min', factor=params.lr_decay)
    bucket = dp.GradBucket(model)
    losses_tr, losses_ev, metrics_tr, metrics_ev = [], [], [], []
    best_metric_ev, best_loss_ev = float('-inf'), float('inf')
    ema = isinstance(optimizer, Adam) and optimizer.ema_decay is not None
    for epoch in range(params.n_epochs):
        if_eval = (epoch + 1) % params.eval_every == 0                                   # main.py:168
        loss_tr, metric_tr = train(x_tr, y_tr, model, optimizer, loss_fn, metric, params, bucket, if_eval)
        if ema:
            # the averaged weights are what is judged: eval loss and metric, is_best and with it best.pth.tar (the BatchNorm running
            # statistics are the live ones: buffers are not averaged)
            with optimizer.ema_weights():
                loss_ev, metric_ev = evaluate(x_ev, y_ev, model, loss_fn, metric, params, if_eval)
        else:
            loss_ev, metric_ev = evaluate(x_ev, y_ev, model, loss_fn, metric, params, if_eval)
        loss_tr, loss_ev = _mean_over_ranks(loss_tr, params), _mean_over_ranks(loss_ev, params)
        scheduler.step(loss_tr)                                                          # plateau on the TRAIN loss (main.py:174)
        is_best = metric_ev > best_metric_ev
        best_metric_ev = max(best_metric_ev, metric_ev)
        best_loss_ev = min(best_loss_ev, loss_ev)
        if params.rank == 0:
            state = {'epoch': epoch + 1, 'state_dict': model.state_dict(), 'optim_dict': optimizer.state_dict()}
            if ema:
                state['ema_state_dict'] = optimizer.ema_state_dict(model)
            utils.save_checkpoint(state, is_best=is_best, checkpoint=checkpoint_dir(model_dir, params))
            if if_eval:
                tail = ''
                if isinstance(optimizer, Adam) and (optimizer.max_grad_norm is not None or optimizer.skip_nonfinite):
                    stats = optimizer.grad_stats()       # one copy and one synchronisation per epoch
                    tail = ' | grad norm: {:.4g} | skipped {:d}'.format(stats['norm'], stats['skipped'])
                print('epoch {} | train loss: {:05.3f} | eval loss: {:05.3f} | best eval loss: {:05.3f} | '
                      'train metric: {:05.3f} | eval metric: {:05.3f} | best eval metric {:05.3f}'.format(
                          epoch + 1, loss_tr, loss_ev, best_loss_ev, metric_tr, metric_ev, best_metric_ev) + tail, flush=True)
                metrics_tr.append(metric_tr)
                metrics_ev.append(metric_ev)
                np.save(os.path.join(model_dir, 'metrics_tr'), metrics_tr)
                np.save(os.path.join(model_dir, 'metrics_ev'), metrics_ev)
        losses_tr.append(loss_tr)
        losses_ev.append(loss_ev)
        if params.rank == 0:
            np.save(os.path.join(model_dir, 'losses_tr'), losses_tr)
            np.save(os.path.join(model_dir, 'losses_ev'), losses_ev)
    return losses_tr, losses_ev


def load_params(model_dir, args):
    """main.py:227-241 (params.device is decided here, the JSON value is ignored)."""
    params = utils.Params(os.path.join(model_dir, 'params.json'))
    params.device = 'cuda' if torch.cuda.is_available() else 'cpu'
    params.seed = args.seed
    if args.dropout >= 0:
        params.dropout = args.dropout
    if not hasattr(params, 'dropout'):
        params.dropout = 0.0
    params.model = args.model
    params.recon = args.recon
    params.recon_coef = float(args.recon_coef)
    params.eval_every = args.eval_every
    params.train_frac = args.train_frac
    if args.n_epochs:
        params.n_epochs = args.n_epochs
    if args.batch_size:
        params.batch_size = args.batch_size
    params.fix_ckpt_dir = args.fix_ckpt_dir
    params.graph = args.graph
    if getattr(args, 'clip_norm', None) is not None:                                     # the command line wins
        params.clip_norm = args.clip_norm
    elif not hasattr(params, 'clip_norm'):
        params.clip_norm = None
    params.skip_nonfinite = bool(getattr(args, 'skip_nonfinite', False) or getattr(params, 'skip_nonfinite', False))
    if getattr(args, 'ema', None) is not None:                                           # the command line wins
        params.ema_decay = args.ema
    elif not hasattr(params, 'ema_decay'):
        params.ema_decay = None
    params.ema_warmup = bool(getattr(args, 'ema_warmup', False) or getattr(params, 'ema_warmup', False))
    params.use_ema = bool(getattr(args, 'use_ema', False))
    if args.model == 'cnn' and getattr(args, 'cnn_kernels', None) is not None:
        params.cnn_kernels = args.cnn_kernels
    return params


def _cnn_on_hip(params):
    return params.model == 'cnn' and getattr(params, 'cnn_kernels', 'torch') == 'hip'


def synthetic_data(args, params):
    n = args.synthetic
    n_ev = max(params.batch_size, n // 4)
    if args.model in ('cnn', 'capsule'):
        mk = lambda k, first: (synth.images(k, 32, first=first), synth.gtsrb_labels(k, params.n_classes, first=first))
    else:
        if params.darknet_input != 32 * params.n_grid and args.model in ('darkcapsule', 'darkcapsule3'):
            raise SystemExit('darkcapsule needs darknet_input = 32 * n_grid (models.py:393); got %d and %d'
                             % (params.darknet_input, params.n_grid))
        mk = lambda k, first: (synth.images(k, params.darknet_input, first=first),
                               synth.gtsdb_labels(k, params.n_grid, params.n_classes, first=first))
    x_tr, y_tr = mk(n, 0)
    x_ev, y_ev = mk(n_ev, n)
    return x_tr, y_tr, x_ev, y_ev


def augmented_data(args, params, data_dir):
    """--augment: (frame numbers, frame numbers, x_ev, y_ev) in place of (x_tr, y_tr, x_ev, y_ev), and params.augment_source, which
    turns a batch of frame numbers into device tensors (augment.AugmentSource).  The raw frames and their boxes come from
    data_dir/train_raw.p and the signs from --gtsrb, or with --synthetic N from synth.raw_images / raw_boxes / sign_bank.  The eval
    set is not augmented: data_dir/eval.p, or the synthetic eval frames resized with no pastes."""
    if args.model not in ('darknet_d', 'darknet_r', 'darkcapsule', 'darkcapsule2', 'darkcapsule3') or args.mode != 'train':
        raise SystemExit('--augment pastes signs over detector frames: --mode train --model darknet_d|darknet_r|darkcapsule*')
    if args.graph:
        raise SystemExit('--augment --graph: the augmented batches are planned on the host per step; run without --graph')
    if params.device != 'cuda':
        raise SystemExit('--augment runs on hand-written gfx950 kernels only; no GPU is visible')
    side, g, C = int(params.darknet_input), int(params.n_grid), int(params.n_classes)
    if args.synthetic:
        n = args.synthetic
        n_ev = max(params.batch_size, n // 4)
        frames = synth.raw_images(n + n_ev)
        boxes = synth.raw_boxes(frames, C)
        bank = augment.SignBank(*synth.sign_bank(16, C))
        from capsyolo_amd.predict_fns import PackedImages
        ev = PackedImages(frames[n:], params.device)
        x_ev = augment.paste_resize_device(ev, None, np.arange(ev.n), augment.full_rects(ev.hw), None, None, side, side,
                                           'u8').cpu().numpy()
        y_ev = np.stack([augment.label_grid(b[:, 0:4], b[:, 4], hw, side, g, C, True) for b, hw in zip(boxes[n:], ev.hw)])
        frames, boxes = frames[:n], boxes[:n]
    else:
        import pickle
        from capsyolo_amd import build_data
        with open(data_dir + '/train_raw.p', 'rb') as f:
            frames, boxes = pickle.load(f)
        with open(data_dir + config.ev_d, 'rb') as f:
            x_ev, y_ev = pickle.load(f)
        bank = build_data.load_bank(args.gtsrb)
    params.augment_source = augment.AugmentSource(frames, boxes, bank, side, g, C, int(getattr(params, 'add_signs', 0)),
                                                  args.seed, params.device, tiles=getattr(args, 'tile_spec', None))
    idx = np.arange(len(frames))
    return idx, idx.copy(), x_ev, y_ev


def check_class_augment(args):
    """The refusals of --class_augment that need neither the data nor a device."""
    if args.augment:
        raise SystemExit('--class_augment jitters the classifiers\' samples and --augment pastes signs over detector frames: give one')
    if args.model not in ('cnn', 'capsule') or args.mode not in ('train', 'overfit'):
        raise SystemExit('--class_augment shifts and brightens classifier samples: --mode train|overfit --model cnn|capsule')


def class_augmented_data(args, params, data_dir):
    """--class_augment: (sample numbers, sample numbers, x_ev, y_ev) in place of (x_tr, y_tr, x_ev, y_ev), and params.augment_source,
    which turns a batch of sample numbers into jittered device tensors (class_augment.ClassAugmentSource).  The training set is the
    one a plain run would read (data_dir, or --synthetic N) and must be byte-exact (input_pipeline.quantize_if_exact).  train_frac
    keeps the leading sample numbers, as it keeps the leading samples of a plain run."""
    if params.device != 'cuda':
        raise SystemExit('--class_augment runs on hand-written gfx950 kernels only; no GPU is visible')
    if args.synthetic:
        x_tr, y_tr, x_ev, y_ev = synthetic_data(args, params)
    else:
        if args.mode == 'overfit':
            raise SystemExit('--mode overfit needs the real dataset under %s (or use --synthetic 3)' % data_dir)
        x_tr, y_tr, x_ev, y_ev = utils.load_data(data_dir, False, npy=args.npy)
    x_u8 = quantize_if_exact(x_tr)
    if x_u8 is None:
        raise SystemExit('--class_augment keeps the training set on the device as bytes, and this one is not (uint8 - 128) / 128')
    params.augment_source = class_augment.ClassAugmentSource(x_u8, y_tr, args.seed, int(getattr(params, 'aug_max_shift', 4)),
                                                             float(getattr(params, 'aug_max_light', 0.05)), params.device)
    idx = np.arange(len(y_tr))
    return idx, idx.copy(), x_ev, y_ev


def predict_class(args, model, model_dir, data_dir, params):
    """main.py:303-317, 349-356, the class-only branch: `--model cnn|capsule --restore last|best` pushes the test set (`--synthetic
    N`: N synthetic GTSRB-shaped samples, otherwise the pickled (x, y) at data_dir/test.p) through the restored classifier and
    writes recog_pr / recog_acc / recog_auc to <model_dir>/metric_output.txt in the reference's format and key order.  The
    scores stay on the device, where the rank counts behind all three numbers are taken in one call (metrics.recog_report); the
    reference's two curve plots (r_auc.png, r_pr.png) are not drawn."""
    if params.device != 'cuda':
        raise SystemExit('predict mode runs on hand-written gfx950 kernels only; no GPU is visible')
    if args.synthetic:
        x, y = synth.images(args.synthetic, 32), synth.gtsrb_labels(args.synthetic, params.n_classes)
    else:
        import pickle
        with open(data_dir + config.te_d, 'rb') as f:
            x, y = pickle.load(f)
    path = os.path.join(model_dir, args.restore + '.pth.tar')
    print("Restoring parameters from {}".format(path))
    utils.load_checkpoint(path, model, params)
    scores = class_scores_device(np.asarray(x), model, params, batch_size=params.batch_size)
    metric_out = metrics.recog_report(y, scores.reshape(len(y), -1), params)
    with open(os.path.join(model_dir, 'metric_output.txt'), 'w') as text_file:
        for k, v in metric_out.items():
            text_file.write("{}:{}, ".format(k, v))
            print("{}:{}, ".format(k, v))
    return metric_out


def _combined_classifier(args, model_dir):
    """The classifier behind --combine: (model, its directory, its params).  The directory is config.model_dir[--combine] or, with
    --model_dir, the detector directory's sibling <model_dir>/../<name>."""
    class_model_dir = config.model_dir[args.combine] if args.model_dir is None else \
        os.path.join(os.path.dirname(os.path.abspath(model_dir)), args.combine)
    class_args = argparse.Namespace(**dict(vars(args), model=args.combine))
    class_params = load_params(class_model_dir, class_args)
    if class_params.use_ema:
        class_params.use_ema = 'if_present'         # the classifier's averages are used when its checkpoint has them
    class_model = model_loss_predict[args.combine][0](class_params).to(device=class_params.device)
    return class_model, class_model_dir, class_params


def predict(args, model, model_dir, data_dir, params):
    """main.py:293-356: `--model cnn|capsule` is the class-only branch (predict_class).  The combined branch,
    `--model darknet_d|darknet_r --combine cnn|capsule --restore last|best`, runs
    dark_class_pred and writes detect_and_recog_mAP / detect_and_recog_acc to <model_dir>/combine-<name>_metric_output.txt.
    The images are a list of raw HWC uint8 arrays: `--synthetic N` draws them (with labels) from synth, otherwise they come from
    data_dir/test_images.npy (an object array) next to data_dir/test.p.  The classifier's directory is config.model_dir[--combine]
    or, with --model_dir, its sibling <model_dir>/../<name>.  With --draw the images with every box in green, labelled with the
    classifier's class index, are written to <model_dir>/output/<i>.ppm (main.py:358-363); without it nothing is drawn.  No cv2
    is needed.  The detect-only branch (no --combine) is `--mode detect`, see detect()."""
    if args.restore is None:
        raise SystemExit('Must give restore file last/best')                           # main.py:294-296
    if args.model in ('cnn', 'capsule'):
        return predict_class(args, model, model_dir, data_dir, params)
    if args.model not in ('darknet_d', 'darknet_r') or args.combine not in ('cnn', 'capsule'):
        raise SystemExit('predict mode runs --model cnn|capsule, or the combined chain --model darknet_d|darknet_r --combine '
                         'cnn|capsule; the detect-only branch of --model darknet_d|darknet_r is --mode detect')
    class_model, class_model_dir, class_params = _combined_classifier(args, model_dir)
    if args.synthetic:
        x = synth.raw_images(args.synthetic)
        y = synth.gtsdb_labels(args.synthetic, params.n_grid, 43)
    else:
        import pickle
        with open(data_dir + config.te_d, 'rb') as f:
            _, y = pickle.load(f)
        x = list(np.load(data_dir + '/test_images.npy', allow_pickle=True))
    y_hat, output = dark_class_pred(x, model, model_dir, params, class_model, class_model_dir, class_params, args.restore,
                                    batch_size=params.batch_size, draw=args.draw, nms_iou=args.nms,
                                    nms_class_aware=args.nms_class_aware)
    metric_out = {name: fn(y, y_hat, params) for name, fn in combine_metrics.items()}
    with open(os.path.join(model_dir, 'combine-{}_metric_output.txt'.format(args.combine)), 'w') as text_file:
        for k, v in metric_out.items():
            text_file.write("{}:{}, ".format(k, v))
            print("{}:{}, ".format(k, v))
    if args.draw:
        _write_output_images(model_dir, output)
    return metric_out


def _write_output_images(model_dir, images):
    """main.py:358-363: <model_dir>/output/<i>.ppm (binary PPM where the reference writes a JPEG: no encoder is available)."""
    save_dir = os.path.join(model_dir, 'output')
    os.makedirs(save_dir, exist_ok=True)
    for i, image in enumerate(images):
        capsule_interpret.write_ppm(os.path.join(save_dir, str(i) + '.ppm'), image)


def detect(args, model, model_dir, data_dir, params):
    """main.py:319-327, 349-363, the detect-only branch: `--model darknet_d|darknet_r --restore last|best` pushes the raw test
    images through the restored detector (predict_fns.dark_pred with the labels, so at its default confidence threshold 0.5) and
    writes detect_AP / detect_acc to <model_dir>/metric_output.txt in the reference's format and key order, both from one
    threshold sweep (metrics.detect_report), and the images with the predicted boxes in green and the ground truth in red to
    <model_dir>/output/<i>.ppm.  The data are those of the combined branch: `--synthetic N` draws images and labels from synth,
    otherwise data_dir/test_images.npy next to data_dir/test.p.  The precision-recall plots (detect_ap/) are not drawn."""
    if args.model not in ('darknet_d', 'darknet_r'):
        raise SystemExit('detect mode runs the detectors only: --model darknet_d|darknet_r')
    if args.restore is None:
        raise SystemExit('Must give restore file last/best')                           # main.py:294-296
    if params.device != 'cuda':
        raise SystemExit('detect mode runs on hand-written gfx950 kernels only; no GPU is visible')
    if args.synthetic:
        x = synth.raw_images(args.synthetic)
        y = synth.gtsdb_labels(args.synthetic, params.n_grid, params.n_classes)
    else:
        import pickle
        with open(data_dir + config.te_d, 'rb') as f:
            _, y = pickle.load(f)
        x = list(np.load(data_dir + '/test_images.npy', allow_pickle=True))
    if getattr(args, 'tile_spec', None) is not None:
        # --tiles: the merged box list of the windows in image pixels against the ground truth decoded with the images' sizes
        from capsyolo_amd.predict_fns import dark_pred_tiled
        try:
            pr, output = dark_pred_tiled(x, model, model_dir, params, args.restore, args.tile_spec, args.nms, y=y,
                                         batch_size=params.batch_size, draw=True, nms_class_aware=args.nms_class_aware)
        except ValueError as e:
            raise SystemExit('--tiles %s: %s' % (args.tiles, e))
        hw = np.array([np.asarray(im).shape[0:2] for im in x], dtype=np.int64)
        _, g_idx, g_xy, _, g_conf = utils.decode_boxes_device(y, params, hw, 0.0, with_conf=True)
        metric_out = metrics.detect_report_boxes((g_idx, g_xy, g_conf), pr[:3], len(x))
    else:
        y_hat, output = dark_pred(x, model, model_dir, params, args.restore, y=y, batch_size=params.batch_size, draw=True, nms_iou=args.nms,
                                  nms_class_aware=args.nms_class_aware)
        metric_out = metrics.detect_report(y, y_hat, params)
    with open(os.path.join(model_dir, 'metric_output.txt'), 'w') as text_file:
        for k, v in metric_out.items():
            text_file.write("{}:{}, ".format(k, v))
            print("{}:{}, ".format(k, v))
    _write_output_images(model_dir, output)
    return metric_out


def check_nms(args):
    """The refusals of --nms / --nms_class_aware / --per_frame that need neither the data nor a device."""
    if args.nms is None:
        if args.nms_class_aware:
            raise SystemExit('--nms_class_aware belongs to the suppression step: give --nms IOU')
        if args.per_frame:
            raise SystemExit('--per_frame belongs to the suppression step: give --nms IOU')
        return
    if not (0.0 <= args.nms <= 1.0):
        raise SystemExit('--nms %r: the IoU threshold must be in [0, 1]' % (args.nms,))
    if not (args.mode in ('detect', 'serve') or (args.mode == 'predict' and args.combine is not None)):
        raise SystemExit('--nms suppresses detector boxes: --mode detect, --mode predict with --combine, or --mode serve')
    if args.per_frame < 0:
        raise SystemExit('--per_frame %d: at least 0' % args.per_frame)
    if args.per_frame and args.mode != 'serve':
        raise SystemExit('--per_frame caps the boxes of a frame of --mode serve')


def check_tiles(args):
    """The refusals of --tiles and its options that need neither the data nor a device; sets args.tile_spec (a tiles.TileSpec, or None)."""
    from capsyolo_amd.tiles import TileSpec, parse_tiles
    args.tile_spec = None
    if args.tiles is None:
        given = [k for k, on in (('--tile_overlap', args.tile_overlap is not None), ('--tile_full', args.tile_full),
                                 ('--tile_margin', args.tile_margin is not None)) if on]
        if given:
            raise SystemExit('%s belongs to the tiling: give --tiles RxC' % given[0])
        return
    try:
        rows, cols = parse_tiles(args.tiles)
        spec = TileSpec(rows, cols, 0 if args.tile_overlap is None else args.tile_overlap, args.tile_full,
                        2.0 if args.tile_margin is None else args.tile_margin)
    except ValueError as e:
        raise SystemExit('--tiles %s: %s' % (args.tiles, e))
    if args.mode == 'train' and args.augment:
        if args.model not in ('darknet_d', 'darknet_r'):
            raise SystemExit('--tiles trains a detector whose output decodes into boxes: --model darknet_d|darknet_r')
    elif args.mode in ('serve', 'detect'):
        if args.nms is None:
            raise SystemExit('--tiles needs --nms IOU: overlapping windows see the same sign more than once')
    else:
        raise SystemExit('--tiles runs the detector on windows of a frame: --mode serve, --mode detect, or --mode train --augment')
    args.tile_spec = spec


TRACK_DEFAULTS = dict(max_tracks=32, track_iou=0.3, max_misses=2, min_hits=2, track_decay=0.9)


def check_track(args):
    """The refusals of --track and its options that need neither the data nor a device."""
    given = ['--' + k for k in TRACK_DEFAULTS if getattr(args, k) is not None] + (['--no_motion'] if args.no_motion else [])
    if not args.track:
        if given:
            raise SystemExit('%s belongs to the tracker: give --track' % given[0])
        return
    if args.mode != 'serve':
        raise SystemExit('--track follows the boxes of --mode serve from frame to frame')
    for k, v in TRACK_DEFAULTS.items():
        if getattr(args, k) is None:
            setattr(args, k, v)
    if not 1 <= args.max_tracks <= 256:
        raise SystemExit('--max_tracks %d: 1 to 256 track slots' % args.max_tracks)
    from capsyolo_amd._lib import query
    pairs = query('cy_track_max_pairs')          # (host arithmetic of the library: no device)
    if args.max_boxes >= 1 and args.max_boxes * args.max_tracks > pairs:
        raise SystemExit('--max_boxes %d x --max_tracks %d: the tracker holds %d pairs' % (args.max_boxes, args.max_tracks, pairs))
    if not (0.0 <= args.track_iou <= 1.0):
        raise SystemExit('--track_iou %r: the IoU threshold must be in [0, 1]' % (args.track_iou,))
    if args.max_misses < 0:
        raise SystemExit('--max_misses %d: at least 0' % args.max_misses)
    if args.min_hits < 1:
        raise SystemExit('--min_hits %d: at least 1' % args.min_hits)
    if not (0.0 <= args.track_decay <= 1.0):
        raise SystemExit('--track_decay %r: the weight must be in [0, 1]' % (args.track_decay,))


def check_frames(args):
    """The refusals of --frame_format, --yuv_matrix and --device_frames that need neither the data nor a device."""
    given = [k for k, on in (('--frame_format', args.frame_format != 'rgb'), ('--yuv_matrix', args.yuv_matrix is not None),
                             ('--device_frames', args.device_frames)) if on]
    if given and args.mode != 'serve':
        raise SystemExit('%s describes the frames of --mode serve' % given[0])
    if args.yuv_matrix is not None:
        if args.frame_format != 'nv12':
            raise SystemExit('--yuv_matrix converts NV12 frames: give --frame_format nv12')
        from capsyolo_amd import nv12
        if args.yuv_matrix not in nv12.MATRICES:
            raise SystemExit('--yuv_matrix %s: one of %s' % (args.yuv_matrix, ', '.join(sorted(nv12.MATRICES))))


def even_frame(frame):
    """The frame without its last row / column where the side is odd: what an NV12 frame of the [H + H/2, W] form can hold."""
    return np.ascontiguousarray(frame[:frame.shape[0] - frame.shape[0] % 2, :frame.shape[1] - frame.shape[1] % 2])


def check_serve(args):
    """The refusals of --mode serve that need neither the data nor a device."""
    if args.model not in ('darknet_d', 'darknet_r') or args.combine not in ('cnn', 'capsule'):
        raise SystemExit('serve mode runs the two-stage chain: --model darknet_d|darknet_r --combine cnn|capsule')
    if args.restore is None:
        raise SystemExit('Must give restore file last/best')
    if args.max_boxes < 1:
        raise SystemExit('--max_boxes %d: at least one box slot' % args.max_boxes)


def serve(args, model, model_dir, data_dir, params):
    """`--mode serve`: both checkpoints are restored ONCE, then the frames (`--synthetic N`: synth.raw_images, frames of different
    sizes; otherwise data_dir/test_images.npy as in predict mode) go through serve.SignDetector one at a time, each call returning
    the frame's labelled boxes.  Per frame one line (size, boxes kept / found, the boxes' classes) is printed and written to
    <model_dir>/serve_output.txt; at the end the totals and the latency p50 / p90 / max over the frames whose shape had been seen
    before (the first frame of a shape also builds that shape's buffers and, with --graph, its capture) are printed.  Returns the
    totals as a dict.
    `--track`: a serve.SignTracker follows the boxes from frame to frame (`--synthetic N`: the N frames are synth.sign_sequence, one
    size, signs drifting over one background); per frame a second line `frame i: live L | confirmed: id/cls/hits ...` (the confirmed
    tracks in slot order) goes to <model_dir>/tracks_output.txt, and the totals gain tracks_born and tracks_confirmed (ids handed out,
    ids that were confirmed at some frame).  serve_output.txt is what it is without the option.
    `--frame_format nv12 [--yuv_matrix NAME]`: every frame is encoded to NV12 on the host first (nv12.from_rgb; an odd frame loses its
    last row / column, and the frame's line says the size used) and the detector reads it in place.  `--device_frames`: the frame, in
    either format, is uploaded before the timed call and handed over as a device tensor."""
    import contextlib
    import time
    from capsyolo_amd import nv12
    from capsyolo_amd.serve import SignDetector, SignTracker
    check_serve(args)
    check_track(args)
    check_frames(args)
    if params.device != 'cuda':
        raise SystemExit('serve mode runs on hand-written gfx950 kernels only; no GPU is visible')
    class_model, class_model_dir, class_params = _combined_classifier(args, model_dir)
    for m, d, p in ((model, model_dir, params), (class_model, class_model_dir, class_params)):
        path = os.path.join(d, args.restore + '.pth.tar')
        print("Restoring parameters from {}".format(path))
        utils.load_checkpoint(path, m, p)
    if args.synthetic:
        frames = synth.sign_sequence(args.synthetic) if args.track else synth.raw_images(args.synthetic)
    else:
        frames = list(np.load(data_dir + '/test_images.npy', allow_pickle=True))
    tracker = None
    if args.track:
        tracker = SignTracker(int(class_params.n_classes), args.max_boxes, max_tracks=args.max_tracks, iou_th=args.track_iou,
                              max_misses=args.max_misses, min_hits=args.min_hits, decay=args.track_decay, motion=not args.no_motion)
    det = SignDetector(model, params, class_model, class_params, max_boxes=args.max_boxes, graph=args.graph, nms_iou=args.nms,
                       nms_class_aware=args.nms_class_aware, per_frame=args.per_frame, tracker=tracker,
                       tiles=getattr(args, 'tile_spec', None), frame_format=args.frame_format,
                       yuv_matrix=args.yuv_matrix or 'bt601')
    seen, ms = set(), []
    out = dict(frames=0, boxes=0, truncated=0, bad_boxes=0)
    confirmed_ids, tracks_born = set(), 0
    with contextlib.ExitStack() as files:
        text_file = files.enter_context(open(os.path.join(model_dir, 'serve_output.txt'), 'w'))
        tracks_file = files.enter_context(open(os.path.join(model_dir, 'tracks_output.txt'), 'w')) if args.track else None
        for i, frame in enumerate(frames):
            frame = np.asarray(frame)
            given = frame
            if args.frame_format == 'nv12':
                frame = even_frame(frame)               # (the line below says the size used)
                given = nv12.from_rgb(frame, args.yuv_matrix or 'bt601')
            if args.device_frames:
                given = torch.from_numpy(np.ascontiguousarray(given)).to(det.dev)
                torch.cuda.synchronize(det.dev)
            t0 = time.perf_counter()
            res = det.detect(given)
            dt = (time.perf_counter() - t0) * 1e3
            if frame.shape in seen:
                ms.append(dt)
            seen.add(frame.shape)
            line = 'frame {}: {}x{} | boxes: {} of {} | classes: {}'.format(i, frame.shape[0], frame.shape[1], res.n, res.total,
                                                                          ' '.join(str(c) for c in res.classes))
            print(line)
            text_file.write(line + '\n')
            out['frames'] += 1
            out['boxes'] += res.n
            out['truncated'] += int(res.truncated)
            out['bad_boxes'] += res.bad['boxes']
            if tracks_file is not None:
                tr = res.tracks
                line = 'frame {}: live {} | confirmed:{}'.format(i, tr.live, ''.join(
                    ' {}/{}/{}'.format(tr.ids[k], tr.classes[k], tr.hits[k]) for k in np.flatnonzero(tr.confirmed)))
                print(line)
                tracks_file.write(line + '\n')
                confirmed_ids.update(int(v) for v in tr.ids[tr.confirmed])
                tracks_born += tr.births
    lat = np.percentile(ms, [50, 90, 100]) if ms else [float('nan')] * 3
    out.update(latency_frames=len(ms), p50_ms=float(lat[0]), p90_ms=float(lat[1]), max_ms=float(lat[2]))
    if args.track:
        out.update(tracks_born=tracks_born, tracks_confirmed=len(confirmed_ids))
        print('tracks born: {} | confirmed: {}'.format(out['tracks_born'], out['tracks_confirmed']))
    print('frames: {} | boxes: {} | truncated frames: {} | bad boxes: {} | latency over {} frames of a seen shape: p50 {:.3f} ms, '
          'p90 {:.3f} ms, max {:.3f} ms'.format(out['frames'], out['boxes'], out['truncated'], out['bad_boxes'], len(ms), *lat))
    return out


def interpret(args, model, model_dir, data_dir, params):
    """capsule_interpret.py:27-68 as a mode: restore the checkpoint, take sample --index of the eval set (data_dir/eval.p, or of
    `--synthetic N` samples), and write into <model_dir>/img/ the sample (orig.ppm), the 16 x 11 reconstructions <v>-<i>.ppm of its
    labelled capsule with offset i added to component v (the reference's file names; binary PPM, neither cv2 nor a PNG encoder is
    needed), all of them as sweep.npy (uint8 [16,11,32,32,3]) and as one contact sheet sheet.ppm (row v, column i).  Prints the
    sample's label, its predicted class and the squared error of the unperturbed reconstruction."""
    if args.model != 'capsule':
        raise SystemExit('interpret mode decodes capsule vectors: it runs --model capsule only')
    if args.restore is None:
        raise SystemExit('Must give restore file last/best')
    if params.device != 'cuda':
        raise SystemExit('interpret mode runs on hand-written gfx950 kernels only; no GPU is visible')
    if args.synthetic:
        x, y = synth.images(args.synthetic, 32), synth.gtsrb_labels(args.synthetic, params.n_classes)
    else:
        import pickle
        with open(data_dir + config.ev_d, 'rb') as f:
            x, y = pickle.load(f)
    if not 0 <= args.index < len(y):
        raise SystemExit('--index %d: the set has %d samples' % (args.index, len(y)))
    path = os.path.join(model_dir, args.restore + '.pth.tar')
    print("Restoring parameters from {}".format(path))
    utils.load_checkpoint(path, model, params)
    res = capsule_interpret.interpret_sample(model, np.asarray(x[args.index]), int(y[args.index]), params)
    sweep = res['sweep'].cpu().numpy()
    img_dir = os.path.join(model_dir, 'img')
    os.makedirs(img_dir, exist_ok=True)
    capsule_interpret.write_ppm(os.path.join(img_dir, 'orig.ppm'), capsule_interpret.to_bytes(x[args.index]))
    for v in range(sweep.shape[0]):
        for i in range(sweep.shape[1]):
            capsule_interpret.write_ppm(os.path.join(img_dir, '%d-%d.ppm' % (v, i)), sweep[v, i])
    np.save(os.path.join(img_dir, 'sweep.npy'), sweep)
    capsule_interpret.write_ppm(os.path.join(img_dir, 'sheet.ppm'), capsule_interpret.contact_sheet(sweep))
    print('sample {} | label: {} | predicted: {} | sqerr: {:.6f}'.format(args.index, res['label'], res['pred'], res['sqerr']))
    return res


def check_attack(args):
    """The refusals of --mode attack that need neither the data nor a device; returns the --eps levels (grey levels, as given)."""
    from capsyolo_amd import attack as image_attack
    if args.model not in ('cnn', 'capsule'):
        raise SystemExit('attack mode differentiates the classifiers with respect to the image: %s; got --model %s'
                         % (image_attack.SUPPORTED, args.model))
    if args.restore is None:
        raise SystemExit('Must give restore file last/best')
    if args.eps is None:
        raise SystemExit('attack mode needs --eps E0,E1,... (grey levels, e.g. 0,1,2,4,8)')
    try:
        levels = image_attack.parse_grey_levels(args.eps)
        if args.attack_alpha is not None:
            image_attack.parse_grey_levels(args.attack_alpha, '--attack_alpha')
    except ValueError as e:
        raise SystemExit(str(e))
    if args.attack == 'pgd' and args.attack_steps < 1:
        raise SystemExit('--attack_steps %d: at least one step' % args.attack_steps)
    if getattr(args, 'index_given', False) and args.index < 0:
        raise SystemExit('--index %d: at least 0' % args.index)
    return levels


def attack(args, model, model_dir, data_dir, params):
    """`--mode attack`: the restored classifier's accuracy on the test set (`--synthetic N`: N synthetic GTSRB-shaped samples,
    otherwise data_dir/test.p) with every image moved inside an L-infinity ball of --eps grey levels by FGSM, or by --attack pgd with
    --attack_steps steps of --attack_alpha grey levels (default 2.5 * eps / steps), against the margin loss (capsule, without the
    reconstruction term) or the cross-entropy (cnn).  Writes `level:accuracy, ` per level, in the format of metric_output.txt, to
    <model_dir>/attack_output.txt and returns {level: accuracy}.  --index I: sample I as it is, at the largest level, and the
    saliency map of its gradient (grey, 0..255 of the image's own maximum) go to attack_<I>_clean.ppm / _adv.ppm / _saliency.ppm."""
    from capsyolo_amd import attack as image_attack
    levels = check_attack(args)
    if args.model == 'cnn' and not _cnn_on_hip(params):
        raise SystemExit('attack mode runs on the project\'s kernels: %s' % image_attack.SUPPORTED)
    if params.device != 'cuda':
        raise SystemExit('attack mode runs on hand-written gfx950 kernels only; no GPU is visible')
    if args.synthetic:
        x, y = synth.images(args.synthetic, 32), synth.gtsrb_labels(args.synthetic, params.n_classes)
    else:
        import pickle
        with open(data_dir + config.te_d, 'rb') as f:
            x, y = pickle.load(f)
    x, y = np.asarray(x), np.asarray(y)
    if getattr(args, 'index_given', False) and args.index >= len(y):
        raise SystemExit('--index %d: the set has %d samples' % (args.index, len(y)))
    path = os.path.join(model_dir, args.restore + '.pth.tar')
    print("Restoring parameters from {}".format(path))
    utils.load_checkpoint(path, model, params)
    params.recon = False                                     # the attacked loss is the classification loss
    loss_fn = model_loss_predict[args.model][1]
    g = image_attack.GREY

    def how(level):
        """(attack, alpha, steps) at one level, in input units; a PGD whose step would be 0 is the single step."""
        alpha = (args.attack_alpha if args.attack_alpha is not None else 2.5 * level / args.attack_steps) * g
        return (args.attack, alpha, args.attack_steps) if args.attack == 'pgd' and alpha > 0 else ('fgsm', None, 0)
    out = {}
    for level in levels:
        kind, alpha, steps = how(level)
        out[level] = image_attack.robust_accuracy(model, x, y, params, loss_fn, [level * g], attack=kind, alpha=alpha, steps=steps,
                                                  batch_size=params.batch_size)[level * g]
    with open(os.path.join(model_dir, 'attack_output.txt'), 'w') as text_file:
        for k, v in out.items():
            text_file.write("{:g}:{}, ".format(k, v))
            print("{:g}:{}, ".format(k, v))
    if getattr(args, 'index_given', False):
        i, level = args.index, max(levels)
        xi = torch.from_numpy(np.ascontiguousarray(x[i:i + 1])).to(device=params.device, dtype=torch.float32).permute(0, 3, 1, 2).contiguous()
        yi = torch.from_numpy(np.ascontiguousarray(y[i:i + 1])).to(device=params.device, dtype=torch.int64)
        kind, alpha, steps = how(level)
        model.eval()
        if kind == 'fgsm':
            adv = image_attack.fgsm(model, xi, yi, params, loss_fn, level * g)
        else:
            adv = image_attack.pgd(model, xi, yi, params, loss_fn, level * g, alpha, steps)
        sal = image_attack.saliency(model, xi, yi, params, loss_fn)[0].cpu().numpy()
        stem = os.path.join(model_dir, 'attack_%d_' % i)
        capsule_interpret.write_ppm(stem + 'clean.ppm', capsule_interpret.to_bytes(x[i]))
        capsule_interpret.write_ppm(stem + 'adv.ppm', capsule_interpret.to_bytes(adv[0].permute(1, 2, 0).cpu().numpy()))
        capsule_interpret.write_ppm(stem + 'saliency.ppm', np.ascontiguousarray(np.repeat(sal[:, :, None], 3, axis=2)))
    return out


def main(argv=None):
    args = parser.parse_args(argv)
    if args.model not in config.model_names:
        print("Did not recognize model, choose from: ", *config.model_names)
        sys.exit()
    if args.class_augment:
        check_class_augment(args)
    if args.mode == 'serve':
        check_serve(args)
    if args.mode == 'attack':
        check_attack(args)
    check_nms(args)
    check_tiles(args)
    check_track(args)
    check_frames(args)
    data_dir, model_dir = config.data_dir[args.model], config.model_dir[args.model]
    if args.model_dir is not None:
        model_dir = args.model_dir
    params = load_params(model_dir, args)
    if args.model == 'cnn' and not _cnn_on_hip(params) and params.skip_nonfinite:
        raise SystemExit('--skip_nonfinite needs the project\'s Adam (capsyolo_amd.optim.Adam): the plain-torch cnn baseline trains with '
                         'torch.optim.Adam; use --cnn_kernels hip or another model')
    if params.clip_norm is not None and not (np.isfinite(params.clip_norm) and params.clip_norm > 0):
        raise SystemExit('--clip_norm must be a positive finite number, got %r' % (params.clip_norm,))
    if params.ema_decay is not None:
        if isinstance(params.ema_decay, bool) or not isinstance(params.ema_decay, (int, float)) or \
                not (np.isfinite(params.ema_decay) and 0 < params.ema_decay < 1):
            raise SystemExit('--ema must be a decay in (0, 1), got %r' % (params.ema_decay,))
        if args.model == 'cnn' and not _cnn_on_hip(params):
            raise SystemExit('--ema needs the project\'s Adam (capsyolo_amd.optim.Adam): the plain-torch cnn baseline trains with '
                             'torch.optim.Adam; use --cnn_kernels hip or another model')
    elif params.ema_warmup:
        raise SystemExit('--ema_warmup shapes the schedule of --ema: give --ema D')
    if params.use_ema and args.mode not in ('predict', 'detect', 'serve', 'interpret', 'attack'):
        raise SystemExit('--use_ema runs a restored model on its averaged weights: --mode predict | detect | serve | interpret | attack')
    if args.mode == 'attack' and args.model == 'cnn' and not _cnn_on_hip(params):
        from capsyolo_amd import attack as image_attack
        raise SystemExit('attack mode runs on the project\'s kernels: %s' % image_attack.SUPPORTED)
    if args.nms_class_aware and int(getattr(params, 'n_classes', 0)) == 0:
        raise SystemExit('--nms_class_aware needs a detector with class scores (n_classes > 0 in %s/params.json)' % model_dir)
    params.rank, params.world, local_rank = dp.init_from_env()
    if params.world > 1 and params.batch_size % params.world:
        raise SystemExit('data parallel: batch_size %d is not divisible by the %d ranks' % (params.batch_size, params.world))
    if params.world > 1 and getattr(params, 'sync_bn', False):     # optional params.json key (new; data parallel only)
        from capsyolo_amd import ops as _ops
        _ops.SYNC_BN = True
    if params.device == 'cuda':
        import torch.distributed as dist
        torch.cuda.set_device(dp.local_device_index(local_rank, dist.get_backend() if dist.is_initialized() else 'nccl'))
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if params.device == 'cuda':
        torch.cuda.manual_seed(args.seed)
    elif args.model != 'cnn' or _cnn_on_hip(params):
        raise SystemExit('model %s runs on hand-written gfx950 kernels only; no GPU is visible' % args.model)

    model_cls, loss_fn, predict_fn, metric = model_loss_predict[args.model]
    if args.no_metric:                                                                 # main.py:87,133
        metric = None
    model = model_cls(params).to(device=params.device)
    dp.broadcast_parameters(model)
    if args.fine_tune > 0:
        model.load_weights('./darknet19_weights.npz', 18)                              # main.py:273-278
        for name, param in model.named_parameters():
            if int(name.split('.')[1].split('_')[1]) <= params.fine_tune:
                param.requires_grad = False
    trainable = [p for p in model.parameters() if p.requires_grad]
    torch_cnn = args.model == 'cnn' and not _cnn_on_hip(params)
    optimizer = torch.optim.Adam(trainable, lr=args.lr) if torch_cnn else \
        Adam(trainable, lr=args.lr, max_grad_norm=params.clip_norm, skip_nonfinite=params.skip_nonfinite,
             ema_decay=params.ema_decay, ema_warmup=params.ema_warmup)

    if args.mode in ('train', 'overfit'):
        if args.augment:
            data = augmented_data(args, params, data_dir)
        elif args.class_augment:
            data = class_augmented_data(args, params, data_dir)
        elif args.synthetic:
            data = synthetic_data(args, params)
        else:
            if args.mode == 'overfit':
                raise SystemExit('--mode overfit needs the real dataset under %s (or use --synthetic 3)' % data_dir)
            data = utils.load_data(data_dir, False, npy=args.npy)
        return train_and_evaluate(model, optimizer, loss_fn, metric, params, data, model_dir, restore_file=args.restore)
    if args.augment:
        raise SystemExit('--augment belongs to --mode train')
    modes = {'predict': predict, 'detect': detect, 'serve': serve, 'interpret': interpret, 'attack': attack}
    if args.mode in modes:
        try:
            return modes[args.mode](args, model, model_dir, data_dir, params)
        except utils.NoEmaInCheckpoint as e:
            raise SystemExit(str(e))


if __name__ == '__main__':
    main()
