"""CPU tests of the tracking step (csrc/track.hip, serve.SignTracker / Tracks, the --track options of main.py, synth.sign_sequence):
the exports and query values, the refusals that come before any device work, the known answers and the id discipline of the numpy
restatement tests/track_ref.py, the record unpacking on restatement-made records, and the argument checks."""
import importlib.util
import os
import re

import numpy as np
import pytest

from helpers import REPO

import track_ref as R
from capsyolo_amd import _lib, serve, synth

ARGS = ('count', 'box_xy', 'conf', 'rect', 'scores', 'K', 'C', 'max_tracks', 'iou_th', 'max_misses', 'min_hits', 'decay', 'motion',
        'state', 'record')


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    lib = _lib.load()
    for name, ret in (('cy_track_update', 'int'), ('cy_track_max_pairs', 'int'), ('cy_track_state_bytes', 'long long')):
        assert re.search(r'\b%s %s\(' % (ret, name), header)
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for struct in ('cy_tracks_header_t', 'cy_track_t'):
        assert re.search(r'\}\s*%s;' % struct, header)
    assert 'cy_track_update' in _lib._SIGS and len(_lib._SIGS['cy_track_update']) == len(ARGS) + 1
    assert _lib.ABI_VERSION == 6 and lib.capsyolo_abi_version() == 6
    # 8 bytes a pair: 4096 pairs are 32 KiB of the 48 KiB a launch gets without opting in
    assert _lib.query('cy_track_max_pairs') == 4096
    q = lambda T, C: _lib.query('cy_track_state_bytes', T, C)            # noqa: E731
    assert q(32, 43) == R.state_nbytes(32, 43) and q(1, 1) == R.state_nbytes(1, 1) and q(256, 300) == R.state_nbytes(256, 300)
    assert q(33, 43) > q(32, 43) and q(32, 44) > q(32, 43) and q(32, 43) % 4 == 0
    assert q(0, 43) == 0 and q(32, 0) == 0


def test_record_layouts_agree():
    assert serve.TRACKS_HEADER_DTYPE == R.HEADER and serve.TRACK_DTYPE == R.TRACK
    assert serve.tracks_record_bytes(32, 16) == R.record_nbytes(32, 16) == 32 + 64 * 32 + 4 * 16
    header = open(os.path.join(REPO, 'include', 'capsyolo_hip.h')).read()
    body = re.search(r'typedef struct \{([^{}]*)\}\s*cy_tracks_header_t;', header, re.S).group(1)
    assert re.findall(r'int (\w+);', body) == list(serve.TRACKS_HEADER_DTYPE.names)
    body = re.search(r'typedef struct \{([^{}]*)\}\s*cy_track_t;', header, re.S).group(1)
    assert re.findall(r'(?:double|int|float) (\w+)(?:\[4\])?;', body) == list(serve.TRACK_DTYPE.names)


def _args(**kw):
    """A call with plausible non-null pointers (never dereferenced on the host; the refusals come before the launch)."""
    a = dict(count=8, box_xy=8, conf=8, rect=8, scores=8, K=16, C=43, max_tracks=32, iou_th=0.3, max_misses=2, min_hits=2, decay=0.9,
             motion=1, state=8, record=8)
    a.update(kw)
    return [a[k] for k in ARGS] + [None]


@pytest.mark.parametrize('kw,msg', [(dict(count=None), 'null argument'), (dict(box_xy=None), 'null argument'),
                                    (dict(conf=None), 'null argument'), (dict(rect=None), 'null argument'),
                                    (dict(scores=None), 'null argument'), (dict(state=None), 'null argument'),
                                    (dict(record=None), 'null argument'),
                                    (dict(max_tracks=0), 'max_tracks=0'), (dict(max_tracks=257, K=1), 'max_tracks=257'),
                                    (dict(K=0), 'K=0'), (dict(K=-3), 'K=-3'),
                                    (dict(K=129, max_tracks=32), 'K=129 slots x max_tracks=32 is 4128 pairs'),
                                    (dict(K=17, max_tracks=256), '4352 pairs'), (dict(K=4097, max_tracks=1), '4097 pairs'),
                                    (dict(K=1 << 30, max_tracks=4), '4294967296 pairs'),
                                    (dict(C=0), 'C=0'), (dict(iou_th=float('nan')), 'iou_th=nan'), (dict(iou_th=1.5), 'iou_th=1.5'),
                                    (dict(iou_th=-0.1), 'iou_th=-0.1'), (dict(max_misses=-1), 'max_misses=-1'),
                                    (dict(min_hits=0), 'min_hits=0'), (dict(decay=1.5), 'decay=1.5'), (dict(decay=-0.5), 'decay=-0.5'),
                                    (dict(decay=float('nan')), 'decay=nan'), (dict(motion=2), 'motion=2'),
                                    (dict(state=12), '8-byte aligned'), (dict(record=4), '8-byte aligned')])
def test_entry_point_refuses_bad_arguments(kw, msg):
    with pytest.raises(_lib.HipExtensionError, match='cy_track_update: .*' + re.escape(msg)):
        _lib.call('cy_track_update', *_args(**kw))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('name', sorted(R.known_answers()))
def test_known_answers_of_the_restatement(name):
    seq, expected = R.known_answers()[name]
    results = R.run(seq)
    assert len(results) == len(expected)
    for (st, rec, _), want in zip(results, expected):
        R.check_known(want, rec, seq['T'], seq['K'])
        assert len(rec) == R.record_nbytes(seq['T'], seq['K']) and len(R.state_bytes(st)) == R.state_nbytes(seq['T'], seq['C'])


def test_the_known_ious_are_what_the_cases_say():
    f = np.float64
    assert R.box_iou([0, 0, 10, 10], [3, 0, 13, 10]) == f(70) / f(130)
    assert R.box_iou([0, 0, 3, 3], [0, 0, 4, 5]) == f(9) / f(20) == 0.45
    got = [R.box_iou(a, d) for a in ([0, 0, 10, 10], [4, 0, 14, 10]) for d in ([3, 0, 13, 10], [-4, 0, 6, 10])]
    assert got == [f(70) / f(130), f(60) / f(140), f(90) / f(110), f(20) / f(180)]
    assert R.box_iou([0, 0, 10, 10], [6, 0, 16, 10]) == 0.25 and R.box_iou([18, 0, 28, 10], [24, 0, 34, 10]) == 0.25
    # the motion case: frame 2 at IoU 0.25, frames 3 and 5 at IoU 1 with the predicted box; without motion frame 5 lies apart
    visited = [v['ious'].tolist() for _, _, v in R.run(R.known_answers()['motion'][0])]
    assert visited == [[], [0.25], [1.0], [], [1.0]]
    visited = [v['ious'].tolist() for _, _, v in R.run(R.known_answers()['no_motion'][0])]
    assert visited == [[], [0.25], [0.25], [], [0.0]]


def test_class_votes_follow_the_float32_sums():
    seq, _ = R.known_answers()['class_votes_sum']
    f = np.float32
    st = R.run(seq)[-1][0]
    want = [(f(0.1) + f(0.1)) + f(0.1), (f(0.2) + f(0.5)) + f(0.9), (f(0.9) + f(0.2)) + f(0.1)]
    assert st.evidence[0].tolist() == want
    seq['kw']['decay'] = 0.5
    st = R.run(seq)[-1][0]
    h = f(0.5)
    assert st.evidence[0, 1] == f(h * f(h * f(0.2) + f(0.5)) + f(0.9))


@pytest.mark.parametrize('shape', [(1, 1, 1), (5, 3, 3), (16, 32, 43)])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_ids_increase_and_are_never_reused(shape, seed):
    K, T, C = shape
    seq = R.integer_sequence(K, T, C, 12, 100 * seed + K)
    born, last, seen_dead = 0, 0, set()
    alive = set()
    for st, rec, _ in R.run(seq):
        head, tracks, det_track = R.view(rec, T, K)
        ids = set(tracks['id'][tracks['id'] != 0].tolist())
        assert len(ids) == int(head['live']) == np.count_nonzero(tracks['id'])      # no id twice
        fresh = ids - alive
        assert sorted(fresh) == list(range(last + 1, last + 1 + int(head['births'])))      # births take the next ids, in order
        assert not (fresh & seen_dead) and int(head['deaths']) == len(alive - ids)
        seen_dead |= alive - ids
        alive, last = ids, last + int(head['births'])
        born += int(head['births'])
        assert int(head['next_id']) == last == st.next_id
        assert set(det_track[det_track != 0].tolist()) <= ids
        free = tracks[tracks['id'] == 0]
        assert not free.view(np.uint8).any()                                         # a free slot is all zero
        assert int(head['confirmed']) == np.count_nonzero((tracks['id'] != 0) & (tracks['hits'] >= 2))
    assert born >= 1


@pytest.mark.parametrize('seed', R.FLOAT_SEEDS)
def test_float_sequences_keep_clear_of_every_decision(seed):
    """The precondition of the GPU comparison on float corners, and that something happens in the sequences."""
    seq = R.float_sequence(seed)
    results = R.run(seq)
    ious = np.concatenate([v['ious'] for _, _, v in results])
    gaps = np.concatenate([v['gaps'] for _, _, v in results])
    print('seed %d: %d IoUs, closest to the threshold %.3g, closest pair in a round %.3g' % (seed, len(ious), np.abs(ious - 0.3).min(), gaps.min()))
    assert np.abs(ious - seq['kw']['iou_th']).min() > 1e-9 and gaps.min() > 1e-12
    miss, births = R.events(seq, results)
    assert 5 * miss >= len(results) and 5 * births >= len(results), (miss, births)


# ------------------------------------------------------------------------------------------------ the record on the host
def test_unpack_tracks_and_tracks():
    seq = R.integer_sequence(5, 3, 3, 10, 8)
    for st, rec, _ in R.run(seq):
        head, trk, det_track = serve.unpack_tracks(rec, 3, 5)
        tr = serve.Tracks(rec, 3, 5, min_hits=2)
        live = np.flatnonzero(st.id != 0)
        assert (tr.frame, tr.live, tr.births, tr.deaths, tr.dropped) == tuple(int(head[k]) for k in ('frame', 'live', 'births', 'deaths', 'dropped'))
        assert tr.live == len(live) and tr.slots.tolist() == live.tolist() and tr.ids.tolist() == st.id[live].tolist()
        np.testing.assert_array_equal(tr.boxes_xy, st.xy[live])
        np.testing.assert_array_equal(tr.classes, np.argmax(st.evidence[live], axis=1) if len(live) else np.zeros(0, np.int64))
        np.testing.assert_array_equal(tr.class_scores, st.evidence[live].max(axis=1) if len(live) else np.zeros(0, np.float32))
        np.testing.assert_array_equal(tr.conf, st.conf[live])
        assert tr.hits.tolist() == st.hits[live].tolist() and tr.misses.tolist() == st.misses[live].tolist() and tr.age.tolist() == st.age[live].tolist()
        assert tr.confirmed.tolist() == (st.hits[live] >= 2).tolist() and tr.confirmed.sum() == int(head['confirmed'])
        assert tr.det_track.tolist() == det_track.tolist() and len(tr.det_track) == 5
        for k, s in enumerate(tr.det):
            assert s == -1 or tr.det_track[s] == tr.ids[k]
        assert tr.record is rec
    with pytest.raises(ValueError, match='3 tracks and 5 box slots has 244 bytes, got 243'):
        serve.unpack_tracks(rec[:-1], 3, 5)
    with pytest.raises(ValueError, match='bytes'):
        serve.Tracks(rec, 4, 5, 2)


# ------------------------------------------------------------------------------------------------ argument checks
def test_sign_tracker_checks_its_arguments_before_touching_the_gpu():
    for kw, msg in ((dict(n_classes=0), 'n_classes'), (dict(n_classes=2.5), 'n_classes'), (dict(max_boxes=0), 'max_boxes'),
                    (dict(max_tracks=0), 'max_tracks'), (dict(max_tracks=257, max_boxes=1), 'at most 256'),
                    (dict(max_boxes=129), '129 x 32 pairs'), (dict(iou_th=1.2), 'iou_th'), (dict(iou_th=float('nan')), 'iou_th'),
                    (dict(max_misses=-1), 'max_misses'), (dict(min_hits=0), 'min_hits'), (dict(decay=-0.1), 'decay'),
                    (dict(decay=float('nan')), 'decay'), (dict(min_hits=True), 'min_hits')):
        a = dict(n_classes=43, max_boxes=16)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            serve.SignTracker(**a)
    with pytest.raises(ValueError, match='tracker must be a SignTracker'):
        serve.SignDetector(None, None, None, None, tracker=object())


def _main():
    spec = importlib.util.spec_from_file_location('cy_main_track_host', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_arguments_and_refusals():
    m = _main()
    a = m.parser.parse_args([])
    assert a.track is False and a.no_motion is False and all(getattr(a, k) is None for k in m.TRACK_DEFAULTS)
    m.check_track(a)
    serve_argv = ['--mode', 'serve', '--model', 'darknet_d', '--combine', 'capsule', '--restore', 'last']
    a = m.parser.parse_args(serve_argv + ['--track'])
    m.check_track(a)
    assert (a.max_tracks, a.track_iou, a.max_misses, a.min_hits, a.track_decay, a.no_motion) == (32, 0.3, 2, 2, 0.9, False)
    a = m.parser.parse_args(serve_argv + ['--track', '--max_tracks', '256', '--track_iou', '0', '--max_misses', '0', '--min_hits', '1',
                                          '--track_decay', '1', '--no_motion'])
    m.check_track(a)
    assert (a.max_tracks, a.track_iou, a.max_misses, a.min_hits, a.track_decay, a.no_motion) == (256, 0.0, 0, 1, 1.0, True)
    track = serve_argv + ['--track']
    for argv, flag in ((['--mode', 'train', '--model', 'darknet_d', '--track'], '--track'),
                       (['--mode', 'detect', '--model', 'darknet_d', '--restore', 'last', '--track'], '--track'),
                       (['--mode', 'predict', '--model', 'darknet_d', '--combine', 'capsule', '--restore', 'last', '--track'], '--track'),
                       (['--mode', 'train', '--model', 'darknet_d', '--max_tracks', '8'], '--max_tracks'),
                       (serve_argv + ['--max_tracks', '8'], '--max_tracks'), (serve_argv + ['--track_iou', '0.5'], '--track_iou'),
                       (serve_argv + ['--max_misses', '1'], '--max_misses'), (serve_argv + ['--min_hits', '3'], '--min_hits'),
                       (serve_argv + ['--track_decay', '0.5'], '--track_decay'), (serve_argv + ['--no_motion'], '--no_motion'),
                       (track + ['--max_tracks', '0'], '--max_tracks 0'), (track + ['--max_tracks', '257'], '--max_tracks 257'),
                       (track + ['--max_tracks', '256', '--max_boxes', '17'], '--max_boxes 17 x --max_tracks 256'),
                       (track + ['--track_iou', '1.5'], '--track_iou 1.5'), (track + ['--track_iou', 'nan'], '--track_iou nan'),
                       (track + ['--max_misses', '-1'], '--max_misses -1'), (track + ['--min_hits', '0'], '--min_hits 0'),
                       (track + ['--track_decay', '1.1'], '--track_decay 1.1'), (track + ['--track_decay', '-0.1'], '--track_decay -0.1')):
        with pytest.raises(SystemExit, match=re.escape(flag)):
            m.main(argv)


def test_sign_sequence():
    a, b = synth.sign_sequence(6, 96, 128, seed=3), synth.sign_sequence(6, 96, 128, seed=3)
    assert len(a) == 6 and all(f.shape == (96, 128, 3) and f.dtype == np.uint8 for f in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(x, y) for x, y in zip(synth.sign_sequence(4, 96, 128, seed=3), a))        # a longer one begins with the shorter
    c = synth.sign_sequence(6, 96, 128, seed=4)
    assert not np.array_equal(a[0], c[0])
    moved = [np.count_nonzero((a[i] != a[i + 1]).any(axis=2)) for i in range(5)]
    assert all(0 < m < 96 * 128 // 4 for m in moved)                     # the signs move, the background stays
    assert synth.sign_sequence(2)[0].shape == (120, 160, 3)
    assert len(synth.raw_images(2)) == 2                                 # (untouched: frames of different sizes)
