"""numpy restatement of the tracking step (csrc/track.hip, `cy_track_update`) -- TEST INFRASTRUCTURE ONLY (nothing in the product
imports this).  Plain loops, one pair at a time; boxes in float64 with the IoU of nms_ref.box_iou, class evidence in float32 with
one rounded operation per numpy operation.  The rule is the comment of cy_track_update in include/capsyolo_hip.h.

  empty_state   the all-zero state of T slots and C classes
  update        one frame: (new state, record bytes, visited); visited['ious'] = the IoU of every (live track, live detection) pair,
                visited['gaps'] = per greedy round the differences between neighbouring DIFFERENT IoUs among the candidates that were
                still free (the tests' preconditions that no decision sits on the threshold or on a near-tie read them)
  state_bytes   a state in the byte layout of the kernel's state buffer
  view          (header, tracks, det_track) of record bytes
  run           a whole sequence from the empty state
  generators    the sequences of the tests (the host tests check the restatement on them, the GPU tests the kernel)
"""
import copy

import numpy as np

from nms_ref import box_iou

HEADER = np.dtype([('frame', '<i4'), ('live', '<i4'), ('confirmed', '<i4'), ('births', '<i4'), ('deaths', '<i4'), ('dropped', '<i4'),
                   ('next_id', '<i4'), ('err', '<i4')])
TRACK = np.dtype([('xy', '<f8', (4,)), ('id', '<i4'), ('cls', '<i4'), ('age', '<i4'), ('hits', '<i4'), ('misses', '<i4'), ('det', '<i4'),
                  ('conf', '<f4'), ('score', '<f4')])
# the state buffer: header, T slots, then float32 [T][C]
STATE_HEADER = np.dtype([('frame', '<i4'), ('next_id', '<i4'), ('pad', '<i4', (6,))])
STATE_SLOT = np.dtype([('xy', '<f8', (4,)), ('vel', '<f8', (4,)), ('id', '<i4'), ('age', '<i4'), ('hits', '<i4'), ('misses', '<i4'),
                       ('conf', '<f4'), ('pad', '<i4', (3,))])
assert HEADER.itemsize == 32 and TRACK.itemsize == 64 and STATE_HEADER.itemsize == 32 and STATE_SLOT.itemsize == 96

DEFAULTS = dict(iou_th=0.3, max_misses=2, min_hits=2, decay=0.9, motion=True)


class State(object):
    def __init__(self, T, C):
        self.T, self.C = T, C
        self.frame, self.next_id = 0, 0
        self.xy, self.vel = np.zeros((T, 4), np.float64), np.zeros((T, 4), np.float64)
        self.id, self.age, self.hits, self.misses = (np.zeros(T, np.int32) for _ in range(4))
        self.conf = np.zeros(T, np.float32)
        self.evidence = np.zeros((T, C), np.float32)


def empty_state(T, C):
    return State(T, C)


def state_nbytes(T, C):
    return STATE_HEADER.itemsize + STATE_SLOT.itemsize * T + 4 * T * C


def record_nbytes(T, K):
    return HEADER.itemsize + TRACK.itemsize * T + 4 * K


def state_bytes(st):
    head = np.zeros(1, STATE_HEADER)
    head['frame'], head['next_id'] = st.frame, st.next_id
    slots = np.zeros(st.T, STATE_SLOT)
    for k in ('xy', 'vel', 'id', 'age', 'hits', 'misses', 'conf'):
        slots[k] = getattr(st, k)
    return np.concatenate([head.view(np.uint8), slots.view(np.uint8), np.ascontiguousarray(st.evidence).view(np.uint8).reshape(-1)])


def view(record, T, K):
    buf = np.asarray(record, dtype=np.uint8).reshape(-1)
    assert buf.size == record_nbytes(T, K)
    a, b = HEADER.itemsize, HEADER.itemsize + TRACK.itemsize * T
    return buf[:a].view(HEADER)[0], buf[a:b].view(TRACK), buf[b:].view('<i4')


def update(state, count, box_xy, conf, rect, scores, iou_th=0.3, max_misses=2, min_hits=2, decay=0.9, motion=True):
    st = copy.deepcopy(state)
    T, C = st.T, st.C
    xy = np.asarray(box_xy, dtype=np.float64).reshape(-1, 4)
    K = len(xy)
    conf = np.asarray(conf, dtype=np.float32).reshape(K)
    rect = np.asarray(rect, dtype=np.int32).reshape(K, 4)
    scores = np.asarray(scores, dtype=np.float32).reshape(K, C)
    iou_th, decay = np.float64(iou_th), np.float32(decay)
    n = min(max(int(count), 0), K)
    det_live = [s for s in range(K) if s < n and rect[s].any()]
    trk_live = [t for t in range(T) if st.id[t] != 0]
    # 2, 3: predicted boxes and candidate pairs
    ious, cand = [], {}
    for t in trk_live:
        p = st.xy[t] + st.vel[t] if motion else st.xy[t]
        for s in det_live:
            iou = box_iou(p, xy[s])
            ious.append(iou)
            if iou > iou_th:                                             # (False for a NaN)
                cand[(t, s)] = iou
    # 4: greedy assignment
    match, taken, gaps = {}, set(), []
    while True:
        free = [(v, t, s) for (t, s), v in cand.items() if t not in match and s not in taken]
        if not free:
            break
        vals = np.unique(np.array([v for v, _, _ in free], dtype=np.float64))
        gaps.extend(np.diff(vals))
        best = max(v for v, _, _ in free)
        t, s = min((t, s) for v, t, s in free if v == best)             # the lower track, then the lower detection
        match[t] = s
        taken.add(s)
    det_of = np.zeros(T, np.int32)
    det_track = np.zeros(K, np.int32)
    deaths = 0
    # 5, 6
    for t in trk_live:
        if t in match:
            s = match[t]
            st.vel[t] = xy[s] - st.xy[t]
            st.xy[t] = xy[s]
            st.conf[t] = conf[s]
            st.hits[t] += 1
            st.misses[t] = 0
            det_of[t] = s
            kept = decay * st.evidence[t]
            st.evidence[t] = kept + scores[s]
            det_track[s] = st.id[t]
        else:
            st.misses[t] += 1
            det_of[t] = -1
            if motion:
                st.xy[t] = st.xy[t] + st.vel[t]
            if st.misses[t] > max_misses:
                for k in ('xy', 'vel', 'id', 'age', 'hits', 'misses', 'conf', 'evidence'):
                    getattr(st, k)[t] = 0
                det_of[t] = 0
                deaths += 1
    # 7
    births = dropped = 0
    for s in det_live:
        if s in taken:
            continue
        free = [t for t in range(T) if st.id[t] == 0]
        if not free:
            dropped += 1
            continue
        t = free[0]
        st.next_id += 1
        st.id[t] = st.next_id
        st.xy[t], st.vel[t], st.conf[t] = xy[s], 0.0, conf[s]
        st.hits[t], st.misses[t], st.age[t] = 1, 0, 0
        st.evidence[t] = scores[s]
        det_of[t] = s
        det_track[s] = st.id[t]
        births += 1
    # 8, 9
    head, tracks = np.zeros(1, HEADER), np.zeros(T, TRACK)
    for t in range(T):
        if st.id[t] == 0:
            continue
        st.age[t] += 1
        with np.errstate(invalid='ignore'):
            c = int(np.argmax(st.evidence[t]))
        r = tracks[t]
        r['xy'], r['id'], r['cls'], r['age'], r['hits'], r['misses'] = st.xy[t], st.id[t], c, st.age[t], st.hits[t], st.misses[t]
        r['det'], r['conf'], r['score'] = det_of[t], st.conf[t], st.evidence[t, c]
    st.frame += 1
    live = st.id != 0
    head['frame'], head['live'], head['confirmed'] = st.frame, live.sum(), (live & (st.hits >= min_hits)).sum()
    head['births'], head['deaths'], head['dropped'], head['next_id'] = births, deaths, dropped, st.next_id
    record = np.concatenate([head.view(np.uint8), tracks.view(np.uint8), det_track.view(np.uint8)])
    return st, record, dict(ious=np.asarray(ious, np.float64), gaps=np.asarray(gaps, np.float64))


# ------------------------------------------------------------------------------------------------ sequences
GOOD_RECT = (1, 2, 1, 2)


def frame(boxes, K, C, scores=None, conf=None, count=None, bad=()):
    """One frame's device arrays (count, box_xy [K, 4], conf [K], rect [K, 4], scores [K, C]) from a list of boxes; the slots in `bad`
    get a zero rect; scores: per box a list of C values (default: class 0 gets 1)."""
    xy, cf, rc, sc = np.zeros((K, 4), np.float64), np.zeros(K, np.float32), np.zeros((K, 4), np.int32), np.zeros((K, C), np.float32)
    for s, b in enumerate(boxes):
        xy[s] = b
        cf[s] = 0.5 + 0.01 * s if conf is None else conf[s]
        if s not in bad:
            rc[s] = GOOD_RECT
        sc[s] = [1.0] + [0.0] * (C - 1) if scores is None else scores[s]
    return (len(boxes) if count is None else count), xy, cf, rc, sc


def run(seq):
    """Per frame (state after it, record bytes, visited), from the empty state."""
    st, out = empty_state(seq['T'], seq['C']), []
    for f in seq['frames']:
        st, rec, vis = update(st, *f, **seq['kw'])
        out.append((st, rec, vis))
    return out


def _seq(K, T, C, frames, **kw):
    return dict(K=K, T=T, C=C, kw=dict(DEFAULTS, **kw), frames=[frame(K=K, C=C, **f) if isinstance(f, dict) else frame(f, K, C) for f in frames])


def known_answers():
    """name -> (sequence, expected): expected[i] = the fields of frame i's record that the case is about, as {field: list}: track
    fields over the slots 0..len-1, 'det_track' over the detection slots, header fields as scalars."""
    A = {}
    A['shift'] = (_seq(2, 2, 3, [[[0, 0, 10, 10]], [[3, 0, 13, 10]]]),
                  [dict(id=[1, 0], hits=[1, 0], births=1), dict(id=[1, 0], hits=[2, 0], age=[2, 0], det=[0, 0], det_track=[1, 0], confirmed=1)])
    # inter 3 x 3 = 9, union 9 + 20 - 9 = 20: the IoU is the double 0.45 itself, and the comparison is strict
    on = [[[0, 0, 3, 3]], [[0, 0, 4, 5]]]
    A['on_threshold'] = (_seq(2, 2, 3, on, iou_th=0.45),
                         [dict(id=[1, 0]), dict(id=[1, 2], misses=[1, 0], hits=[1, 1], det=[-1, 0], det_track=[2, 0], births=1)])
    A['below_threshold'] = (_seq(2, 2, 3, on, iou_th=0.44), [dict(id=[1, 0]), dict(id=[1, 0], hits=[2, 0], det_track=[1, 0], births=0)])
    # A-d0 70/130, B-d0 90/110, A-d1 60/140, B-d1 20/180: B takes d0 first, then A takes d1 (slot order would give A d0)
    A['greedy_not_slot_order'] = (_seq(2, 2, 3, [[[0, 0, 10, 10], [4, 0, 14, 10]], [[3, 0, 13, 10], [-4, 0, 6, 10]]], iou_th=0.3),
                                  [dict(id=[1, 2]), dict(id=[1, 2], det=[1, 0], hits=[2, 2], det_track=[2, 1], births=0)])
    A['tie'] = (_seq(2, 2, 3, [[[0, 0, 10, 10], [0, 0, 10, 10]], [[0, 0, 10, 10]]]),
                [dict(id=[1, 2]), dict(id=[1, 2], det=[0, -1], hits=[2, 1], misses=[0, 1], det_track=[1, 0])])
    mo = [[[0, 0, 10, 10]], [[6, 0, 16, 10]], [[12, 0, 22, 10]], [], [[24, 0, 34, 10]]]
    A['motion'] = (_seq(1, 2, 3, mo, iou_th=0.2, max_misses=2),
                   [dict(id=[1, 0]), dict(id=[1, 0], hits=[2, 0]), dict(id=[1, 0], hits=[3, 0]),
                    dict(id=[1, 0], misses=[1, 0], det=[-1, 0], xy=[[18, 0, 28, 10], [0, 0, 0, 0]]),
                    dict(id=[1, 0], hits=[4, 0], misses=[0, 0], xy=[[24, 0, 34, 10], [0, 0, 0, 0]], next_id=1)])
    A['no_motion'] = (_seq(1, 2, 3, mo, iou_th=0.2, max_misses=2, motion=False),
                      [dict(id=[1, 0]), dict(id=[1, 0], hits=[2, 0]), dict(id=[1, 0], hits=[3, 0]),
                       dict(id=[1, 0], misses=[1, 0], xy=[[12, 0, 22, 10], [0, 0, 0, 0]]),
                       dict(id=[1, 2], misses=[2, 0], hits=[3, 1], det_track=[2], next_id=2)])
    # seen once: never confirmed at min_hits = 2, dead after max_misses + 1 = 3 empty frames, the slot reused under a larger id
    A['flicker'] = (_seq(1, 1, 3, [[[0, 0, 10, 10]], [], [], [], [[0, 0, 10, 10]]]),
                    [dict(id=[1], confirmed=0, live=1), dict(id=[1], misses=[1], confirmed=0), dict(id=[1], misses=[2], confirmed=0),
                     dict(id=[0], live=0, deaths=1, confirmed=0), dict(id=[2], age=[1], hits=[1], births=1, confirmed=0)])
    A['full'] = (_seq(3, 2, 3, [[[0, 0, 10, 10], [20, 0, 30, 10], [40, 0, 50, 10]]]),
                 [dict(id=[1, 2], det_track=[1, 2, 0], dropped=1, births=2, live=2)])
    # slot 1 is inside the live range with a zero rect: it neither matches the track under it nor is born
    A['bad_slot'] = (_seq(3, 4, 3, [dict(boxes=[[0, 0, 10, 10], [20, 0, 30, 10]]),
                                    dict(boxes=[[0, 0, 10, 10], [20, 0, 30, 10], [40, 0, 50, 10]], bad=(1,))]),
                     [dict(id=[1, 2, 0, 0]), dict(id=[1, 2, 3, 0], misses=[0, 1, 0, 0], det=[0, -1, 2, 0], det_track=[1, 0, 3], births=1)])
    box = [[0, 0, 10, 10]]
    # class 2 in the first frame, class 1 in the next two.  decay 1: the sums are (0.1, 0.2, 0.9), (0.2, 0.7, 1.1), (0.3, 1.6, 1.2);
    # decay 0: the last frame alone
    votes = [dict(boxes=box, scores=[[0.1, 0.2, 0.9]]), dict(boxes=box, scores=[[0.1, 0.5, 0.2]]), dict(boxes=box, scores=[[0.1, 0.9, 0.1]])]
    A['class_votes_sum'] = (_seq(1, 1, 3, votes, decay=1.0), [dict(cls=[2]), dict(cls=[2]), dict(cls=[1])])
    A['class_votes_last'] = (_seq(1, 1, 3, votes, decay=0.0), [dict(cls=[2]), dict(cls=[1]), dict(cls=[1], score=[np.float32(0.9)])])
    A['class_tie_nan'] = (_seq(2, 2, 4, [dict(boxes=[[0, 0, 10, 10], [20, 0, 30, 10]], scores=[[0.5, 2.0, 2.0, 1.0], [3.0, 1.0, np.nan, np.nan]])]),
                          [dict(cls=[1, 2], score=[np.float32(2.0), np.float32(np.nan)])])
    return A


def check_known(expected, record, T, K):
    """Assert one frame's expectation on its record bytes."""
    head, tracks, det_track = view(record, T, K)
    for key, want in expected.items():
        if key in HEADER.names:
            assert int(head[key]) == want, (key, int(head[key]), want)
        elif key == 'det_track':
            assert det_track[:len(want)].tolist() == list(want), (key, det_track.tolist(), want)
        else:
            got = tracks[key][:len(want)]
            np.testing.assert_array_equal(got, np.asarray(want, dtype=got.dtype), err_msg=key)


def integer_sequence(K, T, C, n_frames, seed):
    """Boxes with integer corners and integer velocities: every predicted box has integer corners too, so every IoU is an exact
    rational below 2^53 and no decision depends on the arithmetic.  A handful of objects drift, drop out for a frame or two and come
    back, spurious boxes come and go, slots are shuffled, a slot is bad now and then; scores are multiples of 1/8 with planted ties."""
    rng = np.random.RandomState(seed)
    n_obj = max(1, min(K, T + 2, 12))
    pos = rng.randint(0, 48, (n_obj, 2)).astype(np.int64)
    size = rng.randint(4, 16, (n_obj, 2))
    velo = rng.randint(-2, 3, (n_obj, 2))
    cls = rng.randint(0, C, n_obj)
    frames = []
    for _ in range(n_frames):
        boxes, scores = [], []
        for o in range(n_obj):
            pos[o] += velo[o]
            if rng.rand() < 0.25:                                         # missed in this frame
                continue
            boxes.append([pos[o, 0], pos[o, 1], pos[o, 0] + size[o, 0], pos[o, 1] + size[o, 1]])
            sc = rng.randint(0, 9, C) / 8.0
            sc[cls[o]] += 0.5
            scores.append(sc)
        for _ in range(rng.randint(0, 3)):                                # spurious boxes
            a, b = rng.randint(0, 64, 2), rng.randint(0, 64, 2)
            boxes.append([min(a[0], b[0]), min(a[1], b[1]), max(a[0], b[0]), max(a[1], b[1])])
            scores.append(rng.randint(0, 9, C) / 8.0)
        order = rng.permutation(len(boxes))[:K]
        boxes, scores = [boxes[i] for i in order], [scores[i] for i in order]
        bad = tuple(s for s in range(len(boxes)) if rng.rand() < 0.08)
        frames.append(dict(boxes=boxes, scores=scores, conf=(rng.randint(1, 200, max(len(boxes), 1)) / 200.0), bad=bad))
    return _seq(K, T, C, frames)


def float_sequence(seed, K=16, T=32, C=43, n_frames=12):
    """Drifting, jittered boxes with float corners: 6 signs of 20..40 pixels move at up to 3 pixels a frame with a jitter of 1 pixel per
    corner, each is missed in a frame with probability 0.2, and a fresh sign appears with probability 0.3 per frame."""
    rng = np.random.RandomState(seed)
    objs = [[rng.uniform(40, 560, 2), rng.uniform(20, 40, 2), rng.uniform(-3, 3, 2)] for _ in range(6)]
    frames = []
    for _ in range(n_frames):
        if rng.rand() < 0.3:
            objs.append([rng.uniform(40, 560, 2), rng.uniform(20, 40, 2), rng.uniform(-3, 3, 2)])
        boxes, scores = [], []
        for c, wh, v in objs:
            c += v
            if rng.rand() < 0.2:
                continue
            boxes.append(np.concatenate([c - wh / 2, c + wh / 2]) + rng.normal(0.0, 1.0, 4))
            scores.append(rng.uniform(0.0, 1.0, C))
        order = rng.permutation(len(boxes))[:K]
        frames.append(dict(boxes=[boxes[i] for i in order], scores=[scores[i] for i in order], conf=rng.uniform(0.5, 1.0, max(len(boxes), 1))))
    return _seq(K, T, C, frames)


FLOAT_SEEDS = (1, 2, 4, 5, 6)      # chosen on the restatement: the tests' preconditions (threshold, near-ties, misses, births) hold


def events(seq, results):
    """(frames in which a live track went without a detection or died, frames with a birth) of run(seq)."""
    miss = births = 0
    for _, rec, _ in results:
        head, tracks, _ = view(rec, seq['T'], seq['K'])
        miss += bool(((tracks['id'] != 0) & (tracks['misses'] > 0)).any() or head['deaths'] > 0)
        births += bool(head['births'] > 0)
    return miss, births
