"""GPU tests of the tracking step (csrc/track.hip behind serve.SignTracker, `SignDetector(tracker=)`, `main.py --mode serve --track`).
The yardstick is the numpy restatement tests/track_ref.py: the kernel is driven frame by frame with crafted device arrays, and after
every frame the record AND the state buffer are compared with it bit for bit."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import REPO, make_params

import track_ref as R
from capsyolo_amd import models, predict_fns, serve, synth, utils

pytestmark = pytest.mark.gpu


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def _tracker(seq):
    kw = seq['kw']
    return serve.SignTracker(seq['C'], seq['K'], max_tracks=seq['T'], iou_th=kw['iou_th'], max_misses=kw['max_misses'],
                             min_hits=kw['min_hits'], decay=kw['decay'], motion=kw['motion'])


def _drive(trk, frames):
    """[(record bytes, state bytes)] of the kernel, one launch per frame on the tracker's state as it stands."""
    out = []
    stream = torch.cuda.current_stream().cuda_stream
    for count, xy, conf, rect, scores in frames:
        d = [_dev([count], np.int32), _dev(xy, np.float64), _dev(conf, np.float32), _dev(rect, np.int32), _dev(scores, np.float32)]
        trk.launch(*[t.data_ptr() for t in d], stream)
        out.append((trk.record.cpu().numpy(), trk.state.cpu().numpy()))
    return out


def _check(seq, results=None):
    """Kernel = restatement after every frame of the sequence, from the empty state.  Returns the restatement's results."""
    results = R.run(seq) if results is None else results
    got = _drive(_tracker(seq), seq['frames'])
    for i, ((st, rec, _), (g_rec, g_state)) in enumerate(zip(results, got)):
        if not np.array_equal(g_rec, rec):
            head, trk, det_track = R.view(g_rec, seq['T'], seq['K'])
            w_head, w_trk, w_det = R.view(rec, seq['T'], seq['K'])
            raise AssertionError('frame %d: header %s, wanted %s\ntracks %s\nwanted %s\ndet_track %s, wanted %s'
                                 % (i, head, w_head, trk[trk['id'] != 0], w_trk[w_trk['id'] != 0], det_track, w_det))
        np.testing.assert_array_equal(g_state, R.state_bytes(st), err_msg='state after frame %d' % i)
    return results


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('name', sorted(R.known_answers()))
def test_known_answers(name):
    seq, expected = R.known_answers()[name]
    for (_, rec, _), want in zip(_check(seq), expected):
        R.check_known(want, rec, seq['T'], seq['K'])


# (16, 256, 3) and (64, 64, 3) sit at the pair cap of 4096; (8, 8, 300) has more classes than the block has threads
@pytest.mark.parametrize('K,T,C', [(1, 1, 1), (5, 3, 3), (16, 32, 43), (16, 256, 3), (64, 64, 3), (8, 8, 300)])
def test_integer_sequences(K, T, C):
    seq = R.integer_sequence(K, T, C, 10, K + T)
    results = _check(seq)
    miss, births = R.events(seq, results)
    head = R.view(results[-1][1], T, K)[0]
    print('%d frames with a miss, %d with a birth; last header %s' % (miss, births, head))
    assert miss >= 2 and births >= 2
    if (K, T) == (5, 3):
        assert sum(int(R.view(rec, T, K)[0]['dropped']) for _, rec, _ in results) > 0          # more detections than slots


def test_count_above_k_zero_and_negative():
    K, T, C = 4, 6, 3
    rng = np.random.RandomState(5)
    boxes = [[10 * s, 0, 10 * s + 8, 8] for s in range(K)]
    full = dict(boxes=boxes, scores=rng.randint(0, 9, (K, C)) / 8.0)
    frames = [dict(full, count=K + 7), dict(full, count=0), dict(full, count=-3), dict(full, count=2), dict(full, count=1 << 30)]
    seq = R._seq(K, T, C, frames, max_misses=1)
    results = _check(seq)
    heads = [R.view(rec, T, K)[0] for _, rec, _ in results]
    assert [int(h['live']) for h in heads] == [4, 4, 0, 2, 4] and [int(h['births']) for h in heads] == [4, 0, 0, 2, 2]
    assert [int(h['deaths']) for h in heads] == [0, 0, 4, 0, 0] and int(heads[-1]['next_id']) == 8


def test_all_empty_sequence_on_an_empty_state():
    seq = R._seq(16, 32, 43, [[], [], []])
    results = _check(seq)
    for i, (st, rec, _) in enumerate(results):
        head, trk, det_track = R.view(rec, 32, 16)
        assert int(head['frame']) == i + 1 and not rec[4:].any() and not R.state_bytes(st)[4:].any()


@pytest.mark.parametrize('seed', R.FLOAT_SEEDS)
def test_float_sequences(seed):
    seq = R.float_sequence(seed)
    results = R.run(seq)
    ious = np.concatenate([v['ious'] for _, _, v in results])
    gaps = np.concatenate([v['gaps'] for _, _, v in results])
    print('seed %d: %d IoUs, closest to the threshold %.3g, closest pair in a round %.3g' % (seed, len(ious), np.abs(ious - 0.3).min(), gaps.min()))
    assert np.abs(ious - seq['kw']['iou_th']).min() > 1e-9, 'precondition: a candidate IoU on the threshold'
    assert gaps.min() > 1e-12, 'precondition: two IoUs of one round too close to order'
    miss, births = R.events(seq, results)
    assert 5 * miss >= len(results) and 5 * births >= len(results), 'precondition: %d misses, %d births' % (miss, births)
    _check(seq, results)


def test_repeatability_and_reset():
    seq = R.float_sequence(R.FLOAT_SEEDS[0])
    trk = _tracker(seq)
    first = _drive(trk, seq['frames'])
    trk.reset()
    assert not trk.state.cpu().numpy().any()
    second = _drive(trk, seq['frames'])
    fresh = _drive(_tracker(seq), seq['frames'])
    for a, b, c in zip(first, second, fresh):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[0], c[0])
        np.testing.assert_array_equal(a[1], c[1])
    tr = trk.fetch()
    head = R.view(first[-1][0], seq['T'], seq['K'])[0]
    assert (tr.frame, tr.live) == (int(head['frame']), int(head['live'])) and tr.frame == len(seq['frames'])


# ------------------------------------------------------------------------------------------------ the pipeline
K_PIPE, N_FRAMES = 8, 8


class _Chain(object):
    """The untrained models of tests/test_gpu_serve.py's chain, frames of one camera, and a threshold that lets about half of the
    first frame's 8 boxes through."""

    def __init__(self):
        self.dp = make_params(model='darknet_d', n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
        self.cp = make_params(model='capsule', n_classes=3, device='cuda')
        torch.manual_seed(3)
        self.dark, self.caps = models.DarkNet(self.dp).cuda().eval(), models.CapsuleNet(self.cp).cuda().eval()
        self.frames = synth.sign_sequence(N_FRAMES, 80, 100, seed=41)
        with torch.no_grad():
            y = self.dark(predict_fns.PackedImages(self.frames[:1]).resize(64, to_nchw=True)).data
        conf = np.unique(y[..., 0::5].cpu().numpy())[::-1].astype(np.float64)
        print('confidences of frame 0: %s' % conf)
        assert len(conf) >= 6, 'the detector output has too few distinct confidences: %s' % conf
        self.conf_th = float(conf[3] + conf[4]) / 2

    def detector(self, **kw):
        return serve.SignDetector(self.dark, self.dp, self.caps, self.cp, max_boxes=K_PIPE, conf_th=self.conf_th, **kw)

    def tracker(self):
        return serve.SignTracker(3, K_PIPE, max_tracks=6, iou_th=0.3, max_misses=1, min_hits=2, decay=0.9)


@pytest.fixture(scope='module')
def chain():
    return _Chain()


def test_detector_with_a_tracker_equals_the_restatement(chain):
    plain, trk = chain.detector(), chain.tracker()
    tracked = chain.detector(tracker=trk)
    st = R.empty_state(6, 3)
    matched = 0
    for i, frame in enumerate(chain.frames):
        a, b = plain.detect(frame), tracked.detect(frame)
        assert a.tracks is None and isinstance(b.tracks, serve.Tracks)
        np.testing.assert_array_equal(b.record, a.record)                # the detections' record does not change
        # what the plain detector returned, plus the classifier's scores and the crop rectangles of the same chain on the same frame
        state = plain.states[(1, 80, 100)]
        with torch.no_grad():
            _, scores = plain._device_steps(state)
        torch.cuda.synchronize()
        xy, conf = np.zeros((K_PIPE, 4)), np.zeros(K_PIPE, np.float32)
        xy[:a.n], conf[:a.n] = a.boxes_xy, a.conf
        rect = state.rect.cpu().numpy()
        assert [bool(r.any()) for r in rect[:a.n]] == (a.classes >= 0).tolist()
        st, rec, _ = R.update(st, a.total, xy, conf, rect, scores.cpu().numpy(), iou_th=0.3, max_misses=1, min_hits=2, decay=0.9, motion=True)
        np.testing.assert_array_equal(b.tracks.record, rec, err_msg='frame %d' % i)
        np.testing.assert_array_equal(trk.state.cpu().numpy(), R.state_bytes(st), err_msg='state after frame %d' % i)
        assert b.tracks.frame == i + 1 and b.tracks.det_track.shape == (K_PIPE,)
        matched += int((b.tracks.hits >= 2).sum())
        print('frame %d: %d boxes, tracks %s hits %s' % (i, a.n, b.tracks.ids.tolist(), b.tracks.hits.tolist()))
    assert st.next_id >= 1 and matched >= 1, 'nothing was followed: the test shows nothing'
    with pytest.raises(ValueError, match='one frame per call'):
        tracked.detect(chain.frames[:2])
    assert trk.fetch().frame == N_FRAMES                                  # the refused call did not count as a frame


def test_graph_equals_eager_with_the_state_carried_across_replays(chain):
    eager, graphed = chain.detector(tracker=chain.tracker()), chain.detector(tracker=chain.tracker(), graph=True)
    other = synth.sign_sequence(2, 64, 72, seed=42)                      # another frame shape in the middle: a second graph, the same state
    frames = chain.frames[:4] + other + chain.frames[4:]
    records = []
    for i, frame in enumerate(frames):
        a, b = eager.detect(frame), graphed.detect(frame)
        np.testing.assert_array_equal(b.record, a.record, err_msg='frame %d' % i)
        np.testing.assert_array_equal(b.tracks.record, a.tracks.record, err_msg='tracks of frame %d' % i)
        assert b.tracks.frame == i + 1
        records.append(a.tracks.record)
    np.testing.assert_array_equal(graphed.tracker.state.cpu().numpy(), eager.tracker.state.cpu().numpy())
    assert sorted(graphed.states) == [(1, 64, 72), (1, 80, 100)] and all(s.graph is not None for s in graphed.states.values())
    assert not np.array_equal(records[0][4:], records[-1][4:])


def test_detector_refuses_a_tracker_that_does_not_fit(chain):
    with pytest.raises(ValueError, match='max_boxes=4'):
        chain.detector(tracker=serve.SignTracker(3, 4))
    with pytest.raises(ValueError, match='n_classes=43'):
        chain.detector(tracker=serve.SignTracker(43, K_PIPE))


# ------------------------------------------------------------------------------------------------ the command line
def test_main_serve_mode_with_tracks(tmp_path):
    dp = make_params(model='darknet_d', n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
    cp = make_params(model='capsule', n_classes=43, device='cuda')
    torch.manual_seed(3)
    ddir, cdir = str(tmp_path / 'darknet_d'), str(tmp_path / 'capsule')
    utils.save_checkpoint({'epoch': 0, 'state_dict': models.DarkNet(dp).state_dict()}, False, ddir)
    utils.save_checkpoint({'epoch': 0, 'state_dict': models.CapsuleNet(cp).state_dict()}, False, cdir)
    json.dump(dict(batch_size=4, n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, dropout=0.0),
              open(os.path.join(ddir, 'params.json'), 'w'))
    json.dump(dict(batch_size=8, n_classes=43), open(os.path.join(cdir, 'params.json'), 'w'))
    spec = importlib.util.spec_from_file_location('cy_main_track', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.main(['--mode', 'serve', '--model', 'darknet_d', '--combine', 'capsule', '--synthetic', '5', '--graph', '--model_dir', ddir,
                  '--restore', 'last', '--track', '--max_tracks', '8', '--min_hits', '2'])
    lines = open(os.path.join(ddir, 'serve_output.txt')).read().splitlines()
    assert len(lines) == 5 and [ln.split(':')[0] for ln in lines] == ['frame %d' % i for i in range(5)]
    assert out['frames'] == 5 and out['boxes'] == sum(int(ln.split('boxes: ')[1].split(' of ')[0]) for ln in lines)
    assert all(re.match(r'frame \d+: 120x160 \| boxes: \d+ of \d+ \| classes: [-\d ]*$', ln) for ln in lines), lines
    tracks = open(os.path.join(ddir, 'tracks_output.txt')).read().splitlines()
    assert len(tracks) == 5
    confirmed = set()
    for i, ln in enumerate(tracks):
        mt = re.match(r'frame (\d+): live (\d+) \| confirmed:((?: \d+/\d+/\d+)*)$', ln)
        assert mt and int(mt.group(1)) == i and int(mt.group(2)) <= 8, ln
        for item in mt.group(3).split():
            tid, cls, hits = (int(v) for v in item.split('/'))
            assert 1 <= tid <= out['tracks_born'] and 0 <= cls < 43 and hits >= 2
            confirmed.add(tid)
    assert out['tracks_confirmed'] == len(confirmed) <= out['tracks_born']
    assert tracks[0].endswith('confirmed:')                              # nothing is confirmed by one frame
