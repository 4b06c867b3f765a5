"""Streaming sign detector: camera frames in, labelled boxes out, with no host hop between the two networks.

predict_fns.dark_class_pred scores a whole test set and crosses to the host in the middle of every chunk (box count, decoded boxes
to numpy for utils.crop_rectangles, rectangles up again, the crop kernel's error word).  `SignDetector` runs the same chain --
resize -> detector -> decode -> crops -> classifier -> arg-max -- for a FIXED number of box slots, `max_boxes`: the box list stays in
device memory (`cy_boxes_crop_resize_u8` reads the count there and computes the rectangles itself), the classifier always sees
`max_boxes` crops (dead slots are zero crops; in eval mode every sample is independent, so they cannot affect the live ones), and
`cy_pack_detections` writes everything the host wants into ONE record buffer: one copy to the host and one event wait per call.
Every launch has a shape that depends on the frame shape and `max_boxes` alone, so with graph=True the steps between the frame
upload and the record download are captured once per frame shape in a HIP graph and replayed.

Bad boxes (a corner that is not finite, an empty rectangle after clipping) do not raise as they do in utils.crop_rectangles: a
serving loop must not die on one degenerate box.  They come back with class -1 and are counted in `Detections.bad`.

`SignTracker` (optional, `SignDetector(..., tracker=)`) joins the boxes of successive frames of ONE camera into tracks: one more
launch behind `cy_pack_detections` (`cy_track_update`, the rule is in include/capsyolo_hip.h), whose state stays in device memory and
whose record travels beside the detections' record under the same event wait.  `Detections.tracks` is then a `Tracks`.
"""
import gc

import numpy as np
import torch

from . import nv12, ops
from ._lib import HipExtensionError, call, query
from .tiles import TileSpec

# the record buffer of cy_pack_detections (include/capsyolo_hip.h): cy_detections_header_t, then max_boxes cy_detection_t
HEADER_DTYPE = np.dtype([('total', '<i4'), ('kept', '<i4'), ('crop_err', '<i4'), ('resize_err', '<i4')])
RECORD_DTYPE = np.dtype([('xy', '<f8', (4,)), ('image', '<i4'), ('cls', '<i4'), ('conf', '<f4'), ('score', '<f4')])
assert HEADER_DTYPE.itemsize == 16 and RECORD_DTYPE.itemsize == 48


def record_bytes(max_boxes):
    return HEADER_DTYPE.itemsize + RECORD_DTYPE.itemsize * int(max_boxes)


def unpack_record(buf, max_boxes):
    """(header, records) views of a record buffer (a uint8 array of record_bytes(max_boxes) bytes)."""
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    if buf.size != record_bytes(max_boxes):
        raise ValueError('a record of %d slots has %d bytes, got %d' % (max_boxes, record_bytes(max_boxes), buf.size))
    return buf[:HEADER_DTYPE.itemsize].view(HEADER_DTYPE)[0], buf[HEADER_DTYPE.itemsize:].view(RECORD_DTYPE)


# the record buffer of cy_track_update: cy_tracks_header_t, then max_tracks cy_track_t, then det_track int32 [max_boxes]
TRACKS_HEADER_DTYPE = np.dtype([('frame', '<i4'), ('live', '<i4'), ('confirmed', '<i4'), ('births', '<i4'), ('deaths', '<i4'),
                                ('dropped', '<i4'), ('next_id', '<i4'), ('err', '<i4')])
TRACK_DTYPE = np.dtype([('xy', '<f8', (4,)), ('id', '<i4'), ('cls', '<i4'), ('age', '<i4'), ('hits', '<i4'), ('misses', '<i4'),
                        ('det', '<i4'), ('conf', '<f4'), ('score', '<f4')])
assert TRACKS_HEADER_DTYPE.itemsize == 32 and TRACK_DTYPE.itemsize == 64


def tracks_record_bytes(max_tracks, max_boxes):
    return TRACKS_HEADER_DTYPE.itemsize + TRACK_DTYPE.itemsize * int(max_tracks) + 4 * int(max_boxes)


def unpack_tracks(buf, max_tracks, max_boxes):
    """(header, tracks, det_track) views of a tracker's record buffer (a uint8 array of tracks_record_bytes(...) bytes)."""
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    want = tracks_record_bytes(max_tracks, max_boxes)
    if buf.size != want:
        raise ValueError('a record of %d tracks and %d box slots has %d bytes, got %d' % (max_tracks, max_boxes, want, buf.size))
    a, b = TRACKS_HEADER_DTYPE.itemsize, TRACKS_HEADER_DTYPE.itemsize + TRACK_DTYPE.itemsize * int(max_tracks)
    return buf[:a].view(TRACKS_HEADER_DTYPE)[0], buf[a:b].view(TRACK_DTYPE), buf[b:].view('<i4')


class Tracks(object):
    """The tracks after one frame.  frame: frames since the tracker's reset, this one included; live: tracks alive; births / deaths /
    dropped: tracks born and freed in this frame, detections that found no free slot in it.  Per live track, in slot order: ids int64
    [live] (from 1, never reused), boxes_xy float64 [live, 4], classes int64 (arg-max of the class evidence summed over the track's
    detections), class_scores float32 (that sum), conf float32 (of the last matched detection), age / hits / misses int64, det int64
    (this frame's detection slot, -1: none), confirmed bool (hits >= the tracker's min_hits), slots int64 (the track's slot).
    det_track int64 [max_boxes]: per detection slot the id of its track, 0 for none -- it labels `Detections`' boxes.  record: the
    raw bytes."""

    def __init__(self, record, max_tracks, max_boxes, min_hits):
        head, trk, det_track = unpack_tracks(record, max_tracks, max_boxes)
        self.record = record
        self.frame, self.live = int(head['frame']), int(head['live'])
        self.births, self.deaths, self.dropped = int(head['births']), int(head['deaths']), int(head['dropped'])
        self.slots = np.flatnonzero(trk['id'] != 0).astype(np.int64)
        trk = trk[self.slots]
        self.ids = trk['id'].astype(np.int64)
        self.boxes_xy = np.ascontiguousarray(trk['xy'], dtype=np.float64).reshape(-1, 4)
        self.classes = trk['cls'].astype(np.int64)
        self.class_scores = np.ascontiguousarray(trk['score'], dtype=np.float32)
        self.conf = np.ascontiguousarray(trk['conf'], dtype=np.float32)
        self.age, self.hits, self.misses = (trk[k].astype(np.int64) for k in ('age', 'hits', 'misses'))
        self.det = trk['det'].astype(np.int64)
        self.confirmed = self.hits >= int(min_hits)
        self.det_track = det_track.astype(np.int64)


class SignTracker(object):
    """trk = SignTracker(n_classes, max_boxes, max_tracks=32, iou_th=0.3, max_misses=2, min_hits=2, decay=0.9, motion=True, device=None)

    The tracks of one camera for `SignDetector(..., tracker=trk)`: n_classes and max_boxes are the classifier's classes and the
    detector's box slots.  A detection joins the track whose predicted box (with motion: the last box moved on by the last step)
    overlaps it most, at IoU > iou_th, greedily; a track without a detection for more than max_misses frames in a row ends; a
    detection without a track starts one, while one of the max_tracks slots is free; a track counts as confirmed from min_hits
    detections on; its class is the arg-max of sum_k decay^k * (class scores k detections ago).  Owns the state and record buffers on
    the device and a pinned host record; reset() empties the tracks (stream-ordered, ids start again at 1)."""

    def __init__(self, n_classes, max_boxes, max_tracks=32, iou_th=0.3, max_misses=2, min_hits=2, decay=0.9, motion=True, device=None):
        for name, v, lo in (('n_classes', n_classes, 1), ('max_boxes', max_boxes, 1), ('max_tracks', max_tracks, 1),
                            ('max_misses', max_misses, 0), ('min_hits', min_hits, 1)):
            if isinstance(v, bool) or int(v) != v or v < lo:
                raise ValueError('%s must be an integer >= %d, got %r' % (name, lo, v))
        if max_tracks > 256:
            raise ValueError('max_tracks must be at most 256, got %r' % (max_tracks,))
        pairs = query('cy_track_max_pairs')
        if int(max_boxes) * int(max_tracks) > pairs:
            raise ValueError('max_boxes x max_tracks = %d x %d pairs, the tracker holds %d' % (max_boxes, max_tracks, pairs))
        if not (0.0 <= float(iou_th) <= 1.0):
            raise ValueError('iou_th must be in [0, 1], got %r' % (iou_th,))
        if not (0.0 <= float(decay) <= 1.0):
            raise ValueError('decay must be in [0, 1], got %r' % (decay,))
        self.C, self.K, self.T = int(n_classes), int(max_boxes), int(max_tracks)
        self.n_classes, self.max_boxes, self.max_tracks = self.C, self.K, self.T
        self.iou_th, self.max_misses, self.min_hits = float(iou_th), int(max_misses), int(min_hits)
        self.decay, self.motion = float(decay), bool(motion)
        if not torch.cuda.is_available():
            raise HipExtensionError('SignTracker needs the GPU: there is no CPU path')
        self.dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self.dev.type != 'cuda':
            raise ValueError('the tracker lives on a GPU, got device %s' % (self.dev,))
        if self.dev.index is None:
            self.dev = torch.device('cuda', torch.cuda.current_device())
        self.state = torch.zeros(int(query('cy_track_state_bytes', self.T, self.C)), dtype=torch.uint8, device=self.dev)
        nbytes = tracks_record_bytes(self.T, self.K)
        self.record = torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)
        self.record_host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()

    def reset(self):
        """No tracks, frame 0, ids from 1 again: the all-zero state, ordered on the current stream like the launches."""
        self.state.zero_()

    def launch(self, count, box_xy, conf, rect, scores, stream):
        """One frame: device pointers to count[1], box_xy[K][4] (double), conf[K], rect[K][4] (int32), scores[K][C] (float32)."""
        call('cy_track_update', count, box_xy, conf, rect, scores, self.K, self.C, self.T, self.iou_th, self.max_misses, self.min_hits,
             self.decay, int(self.motion), self.state.data_ptr(), self.record.data_ptr(), stream)

    def tracks(self, record=None):
        """`Tracks` of record bytes (default: a copy of the host record as it stands)."""
        return Tracks(self.record_host.numpy().copy() if record is None else record, self.T, self.K, self.min_hits)

    def fetch(self):
        """The device record as `Tracks` (a blocking copy on the current stream: for tools and tests, not for the serving loop)."""
        return self.tracks(self.record.cpu().numpy())


class Detections(object):
    """What one `SignDetector.detect` call found.  n boxes are kept of `total` over the threshold (`truncated`: total > max_boxes,
    the first max_boxes in the decode kernel's order, which is np.argwhere's, are kept); bad = {'boxes': kept boxes without a crop
    (class -1), 'frames': frames the resize refused}; image_indices int64 [n], boxes_xy float64 [n, 4] = (x1, y1, x2, y2) in frame
    pixels, conf float32 [n], classes int64 [n], class_scores float32 [n]; record: the raw bytes all of it was read from.
    From a detector built with nms_iou the record has the same layout, but `total` is the number of boxes that survived the
    suppression step (all boxes over the threshold take part in it, however many), and the boxes come image ascending and inside an
    image confidence descending: a truncated result then holds the most confident survivors of the first images.
    tracks: the `Tracks` after this frame from a detector with a tracker, else None."""

    def __init__(self, record, max_boxes):
        head, rec = unpack_record(record, max_boxes)
        self.record = record
        self.total, self.n = int(head['total']), int(head['kept'])
        self.truncated = self.total > max_boxes
        self.bad = {'boxes': int(head['crop_err']), 'frames': int(head['resize_err'])}
        rec = rec[:self.n]
        self.image_indices = rec['image'].astype(np.int64)
        self.boxes_xy = np.ascontiguousarray(rec['xy'], dtype=np.float64).reshape(-1, 4)
        self.conf = np.ascontiguousarray(rec['conf'], dtype=np.float32)
        self.classes = rec['cls'].astype(np.int64)
        self.class_scores = np.ascontiguousarray(rec['score'], dtype=np.float32)
        self.tracks = None


class _State(object):
    """Every buffer of the pipeline for frames of one shape (n, H, W), or for n NV12 surfaces of one `nv12.Layout`: nothing is
    allocated per call.  The pinned staging buffer belongs to frames that come from the host and is built when the first one does."""

    def __init__(self, n, H, W, side, ci, K, has_cls, dev, tiles=None, layout=None):
        self.layout = layout
        self.frame_bytes = H * W * 3 if layout is None else layout.nbytes
        nbytes = n * self.frame_bytes
        self.n, self.H, self.W, self.nbytes = n, H, W, nbytes
        self.staging, self.staging_np = None, None
        self.frames = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.off = (torch.arange(n, dtype=torch.int64) * self.frame_bytes).to(dev)
        self.hw32 = torch.tensor([[H, W]] * n, dtype=torch.int32).to(dev)
        # the image table of the two crop launches: (H, W) per packed RGB frame, (H, W, pitch, uv_off) per NV12 surface
        self.img_geom = self.hw32 if layout is None else torch.tensor([layout.geom] * n, dtype=torch.int32).to(dev)
        self.hw64 = torch.tensor([[H, W]] * n, dtype=torch.int64).to(dev)
        # the whole-frame resize in front of the detector: frame i, rectangle (0, H, 0, W)
        self.frame_idx = torch.arange(n, dtype=torch.int32).to(dev)
        self.frame_rect = torch.tensor([[0, H, 0, W]] * n, dtype=torch.int32).to(dev)
        self.words = torch.zeros(4, dtype=torch.int32, device=dev)         # box count, crop error word, resize error word, unused
        self.n_dark = n                 # images in front of the detector: the frames, or with tiles every frame's windows
        if tiles is not None:
            # the tile table of this frame shape, frame-major: tile b = rectangle tile_rect[b] of frame tile_idx[b] (ascending)
            rects = tiles.rects(H, W)
            self.n_dark = n * len(rects)
            self.tile_idx = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int32), len(rects))).to(dev)
            self.tile_rect = torch.from_numpy(np.ascontiguousarray(np.tile(rects, (n, 1)))).to(dev)
        self.x_dark = torch.zeros((self.n_dark, 3, side, side), dtype=torch.float32, device=dev)
        self.box_img = torch.zeros(K, dtype=torch.int32, device=dev)
        self.box_xy = torch.zeros((K, 4), dtype=torch.float64, device=dev)
        self.box_conf = torch.zeros(K, dtype=torch.float32, device=dev)
        self.box_cls = torch.zeros(K, dtype=torch.int32, device=dev) if has_cls else None
        self.rect = torch.zeros((K, 4), dtype=torch.int32, device=dev)
        self.crops = torch.zeros((K, 3, ci, ci), dtype=torch.float32, device=dev)
        self.record = torch.zeros(record_bytes(K), dtype=torch.uint8, device=dev)
        self.record_host = torch.zeros(record_bytes(K), dtype=torch.uint8).pin_memory()
        self.done = torch.cuda.Event()
        self.graph, self.graph_key, self.keep = None, None, None
        self.cand = None        # with nms_iou: the candidate list in front of the suppression step (_Candidates, built on first use)


    def stage(self):
        """The pinned host buffer, one row of frame_bytes per frame."""
        if self.staging is None:
            self.staging = torch.empty(self.nbytes, dtype=torch.uint8).pin_memory()
            self.staging_np = self.staging.numpy().reshape(self.n, self.frame_bytes)
        return self.staging_np


class _Candidates(object):
    """The decode kernel's whole output for one frame shape, cap = n g^2 n_boxes entries, and what `cy_nms_boxes` needs beside it."""

    def __init__(self, cap, n, K, has_cls, dev, tiled=False):
        self.cap = cap
        self.img = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.xy = torch.zeros((cap, 4), dtype=torch.float64, device=dev)
        self.conf = torch.zeros(cap, dtype=torch.float32, device=dev)
        self.cls = torch.zeros(cap, dtype=torch.int32, device=dev) if has_cls else None
        self.keep = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.src = torch.zeros(K, dtype=torch.int32, device=dev)            # the survivors' positions in the list
        # candidate count, error word, per-image scratch; with tiles behind them: boxes the border rule dropped, bad tiles
        self.words = torch.zeros(2 + n + (2 if tiled else 0), dtype=torch.int32, device=dev)


class SignDetector(object):
    """det = SignDetector(dark_model, dark_params, class_model, class_params, max_boxes=16, conf_th=0.5, graph=False,
                        nms_iou=None, nms_class_aware=False, per_frame=0, tracker=None, tiles=None, frame_format='rgb',
                        yuv_matrix='bt601')
    res = det.detect(frames)

    dark_model: a DarkNet on the device (dark_params: darknet_input, n_grid, n_classes, capsule_input); class_model: CapsuleNet, or
    the plain-torch ConvNet, on capsule_input x capsule_input crops.  The caller restores the checkpoints; both models are put in
    eval mode and everything runs under no_grad.  frames: one HWC uint8 array, or a list / an [n, H, W, 3] array of frames of ONE size.
    The buffers (and with graph=True the captured graph) are built per frame shape (n, H, W) on first use and kept.  The steps run
    on torch's current stream; the call returns after the record has arrived (one event wait).
    nms_iou (optional): non-maximum suppression between the decode and the crops (`cy_nms_boxes`, the rule is in
    include/capsyolo_hip.h): ALL boxes over conf_th are decoded, and the max_boxes slots take the survivors, most confident first,
    at most per_frame of a frame (0: no cap); nms_class_aware suppresses only inside the detector's own arg-max class and needs a
    detector with class scores.  None: no such step, the first max_boxes boxes in decode order as before.
    tracker (optional): a `SignTracker` for the classifier's classes and max_boxes slots on the detector's device.  Every call is then
    ONE frame of the tracker's camera: `cy_track_update` runs behind the pack step on the same stream (with graph=True inside every
    frame shape's graph, all on the tracker's one state), and the result carries `.tracks`.  The detections' record does not change.
    tiles (optional): a `tiles.TileSpec`.  The detector then sees the T = rows x cols (+ 1 with full) overlapping windows of every
    frame instead of the frame, each resized to darknet_input: one `cy_crop_resize_u8` for all n T windows, the detector on that
    batch, `cy_yolo_decode_tiles_conf` (border rule and shift into frame pixels, include/capsyolo_hip.h) into one candidate list of
    n T g^2 n_boxes entries, `cy_nms_boxes` per frame with room for T g^2 n_boxes boxes (at most cy_nms_max_per_image()).  Needs
    nms_iou: the overlaps show a sign to more than one window by construction.  Crops, classifier, record and tracker are as
    without tiles, on the full frames.  None: the launches are exactly those of a detector without the argument.
    frame_format: 'rgb' (packed HWC uint8, as above) or 'nv12'.  An NV12 frame is a contiguous uint8 [H + H/2, W] array with even H, W
    (the Y plane, then the rows of interleaved U, V pairs), or, with `detect(frames, layout=nv12.Layout(...))`, a 1-D / 2-D buffer of
    layout.nbytes bytes: a decoder surface with a row pitch and a chroma offset of its own.  The frames are uploaded as they are, 1.5
    bytes per pixel, and `cy_crop_resize_nv12` / `cy_boxes_crop_resize_nv12` convert in their tap fetch by the colour rule of
    include/capsyolo_hip.h with the row yuv_matrix (a name of nv12.MATRICES, an nv12.YuvMatrix or six integers); the record is bit
    for bit that of an 'rgb' detector on the frame converted by that rule.  yuv_matrix belongs to 'nv12'.
    Device-resident frames (both formats): detect() also takes a contiguous torch.uint8 tensor on the detector's device, or a list of
    them, of the shapes above.  They are copied device to device into the state's frame buffer on the current stream (a captured
    graph keeps its addresses); no staging buffer, no host copy, no further synchronisation, and the tensor is not kept."""

    def __init__(self, dark_model, dark_params, class_model, class_params, max_boxes=16, conf_th=0.5, graph=False, nms_iou=None,
                 nms_class_aware=False, per_frame=0, tracker=None, tiles=None, frame_format='rgb', yuv_matrix='bt601'):
        if int(max_boxes) != max_boxes or max_boxes < 1:
            raise ValueError('max_boxes must be an integer >= 1, got %r' % (max_boxes,))
        if frame_format not in ('rgb', 'nv12'):
            raise ValueError("frame_format must be 'rgb' or 'nv12', got %r" % (frame_format,))
        if frame_format == 'rgb' and not (isinstance(yuv_matrix, str) and yuv_matrix == 'bt601'):
            raise ValueError("yuv_matrix belongs to frame_format='nv12': packed RGB frames are not converted")
        self.frame_format, self.yuv = frame_format, nv12.coef(yuv_matrix)
        self._coef = nv12.c_coef(self.yuv)
        if nms_iou is not None and not (0.0 <= float(nms_iou) <= 1.0):
            raise ValueError('nms_iou must be in [0, 1], got %r' % (nms_iou,))
        if int(per_frame) != per_frame or per_frame < 0:
            raise ValueError('per_frame must be an integer >= 0, got %r' % (per_frame,))
        if nms_iou is None and (nms_class_aware or per_frame):
            raise ValueError('nms_class_aware and per_frame belong to the suppression step: give nms_iou')
        if nms_class_aware and int(dark_params.n_classes) == 0:
            raise ValueError('nms_class_aware needs a detector with class scores (n_classes > 0)')
        if tiles is not None:
            if not isinstance(tiles, TileSpec):
                raise ValueError('tiles must be a TileSpec, got %r' % (type(tiles).__name__,))
            if nms_iou is None:
                raise ValueError('tiles need nms_iou: overlapping windows see the same sign more than once by construction')
            tiles.check_capacity(dark_params.n_grid, dark_params.n_boxes, query('cy_nms_max_per_image'))
        if tracker is not None:
            if not isinstance(tracker, SignTracker):
                raise ValueError('tracker must be a SignTracker, got %r' % (type(tracker).__name__,))
            if tracker.max_boxes != int(max_boxes):
                raise ValueError('the tracker was built for max_boxes=%d, the detector has %d' % (tracker.max_boxes, max_boxes))
            if tracker.n_classes != int(class_params.n_classes):
                raise ValueError('the tracker was built for n_classes=%d, the classifier has %d' % (tracker.n_classes, class_params.n_classes))
        if not torch.cuda.is_available():
            raise HipExtensionError('SignDetector needs the GPU: there is no CPU path')
        self.dark, self.dark_params, self.cls, self.class_params = dark_model, dark_params, class_model, class_params
        self.K, self.conf_th, self.use_graph = int(max_boxes), float(conf_th), bool(graph)
        self.nms_iou = None if nms_iou is None else float(nms_iou)
        self.nms_class_aware, self.per_frame = bool(nms_class_aware), int(per_frame)
        self.side, self.ci = int(dark_params.darknet_input), int(dark_params.capsule_input)
        self.g, self.C = int(dark_params.n_grid), int(dark_params.n_classes)
        self.dev = next(dark_model.parameters()).device
        if self.dev.type != 'cuda' or next(class_model.parameters()).device != self.dev:
            raise ValueError('both models must be on the same GPU; the detector is on %s' % (self.dev,))
        if tracker is not None and tracker.dev != self.dev:
            raise ValueError('the tracker is on %s, the detector on %s' % (tracker.dev, self.dev))
        self.tracker, self.tiles = tracker, tiles
        for m in (dark_model, class_model):
            if m.training:          # (a switch of mode starts a new fold-cache epoch, which would rebuild other detectors' captures)
                m.eval()
        self._tensors = [t for m in (dark_model, class_model) for t in list(m.parameters()) + list(m.buffers())]
        self.states = {}

    # ------------------------------------------------------------------------------------------------ frames
    @staticmethod
    def _frames(frames):
        if isinstance(frames, np.ndarray) and frames.ndim == 3:
            frames = [frames]
        arrs = [np.asarray(f) for f in frames]
        if not arrs:
            raise ValueError('no frames')
        for k, a in enumerate(arrs):
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError('frame %d: expected a uint8 array [H, W, 3], got %s %s' % (k, a.dtype, a.shape))
            if a.shape != arrs[0].shape:
                raise ValueError('frame %d is %d x %d, frame 0 is %d x %d: one call takes frames of one size'
                                 % (k, a.shape[0], a.shape[1], arrs[0].shape[0], arrs[0].shape[1]))
        return arrs

    def _sources(self, frames, layout=None):
        """(device-resident?, the frames as a list of flat-able arrays or tensors, H, W, layout or None) of one detect() call."""
        fmt = self.frame_format
        if layout is not None:
            if fmt != 'nv12':
                raise ValueError("layout= describes an NV12 surface: the detector was built with frame_format='rgb'")
            if not isinstance(layout, nv12.Layout):
                raise ValueError('layout must be an nv12.Layout, got %r' % (type(layout).__name__,))
        if isinstance(frames, (np.ndarray, torch.Tensor)):
            if layout is not None:
                one = int(np.prod(tuple(frames.shape))) == layout.nbytes and frames.ndim <= 2
            else:
                one = frames.ndim == (3 if fmt == 'rgb' else 2)
            frames = [frames] if one else list(frames)
        items = list(frames)
        if not items:
            raise ValueError('no frames')
        on_dev = [isinstance(f, torch.Tensor) for f in items]
        if any(on_dev) and not all(on_dev):
            raise ValueError('host arrays and device tensors mixed in one call: frame %d is a %s, frame 0 a %s'
                             % (on_dev.index(not on_dev[0]), 'tensor' if not on_dev[0] else 'host array',
                                'tensor' if on_dev[0] else 'host array'))
        if on_dev[0]:
            for k, t in enumerate(items):
                if t.device != self.dev:
                    raise ValueError('frame %d is a tensor on %s, the detector is on %s' % (k, t.device, self.dev))
                if t.dtype != torch.uint8:
                    raise ValueError('frame %d: expected a torch.uint8 tensor, got dtype %s' % (k, t.dtype))
                if not t.is_contiguous():
                    raise ValueError('frame %d is not contiguous: a frame is copied as one run of bytes' % k)
        elif fmt == 'rgb':
            items = self._frames(items)
        else:
            items = [np.asarray(f) for f in items]
            for k, a in enumerate(items):
                if a.dtype != np.uint8:
                    raise ValueError('frame %d: expected a uint8 array, got %s %s' % (k, a.dtype, a.shape))
                if not a.flags['C_CONTIGUOUS']:
                    raise ValueError('frame %d is not contiguous: an NV12 frame is copied as one run of bytes' % k)
        tight = None
        for k, f in enumerate(items):
            shape = tuple(f.shape)
            if fmt == 'rgb':
                if on_dev[0] and (len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1):    # (host frames: _frames did)
                    raise ValueError('frame %d: expected a uint8 tensor [H, W, 3], got shape %s' % (k, shape))
            elif layout is not None:
                if len(shape) not in (1, 2) or int(np.prod(shape)) != layout.nbytes:
                    raise ValueError('frame %d: %r has %d bytes, got a buffer of shape %s' % (k, layout, layout.nbytes, shape))
            else:
                try:
                    tight = nv12.Layout.of(f) if k == 0 else tight
                except ValueError as e:
                    raise ValueError('frame %d: %s (or give layout=)' % (k, e))
            if shape != tuple(items[0].shape):
                raise ValueError('frame %d has shape %s, frame 0 has %s: one call takes frames of one size' % (k, shape, tuple(items[0].shape)))
        if fmt == 'rgb':
            H, W = items[0].shape[0:2]
        else:
            layout = tight if layout is None else layout
            H, W = layout.H, layout.W
        return on_dev[0], items, int(H), int(W), layout

    def _state(self, n, H, W, layout=None):
        key = (n, H, W) if layout is None else (n, layout)
        if key not in self.states:
            self.states[key] = _State(n, H, W, self.side, self.ci, self.K, self.C > 0, self.dev, self.tiles, layout)
        return self.states[key]

    def _images(self, st):
        """The entry-point suffix and the leading arguments of the two crop launches: where the frames lie and what they are."""
        head = (st.frames.data_ptr(), st.off.data_ptr(), st.img_geom.data_ptr(), st.n, st.nbytes)
        return ('u8', head) if st.layout is None else ('nv12', head + (self._coef,))

    # ------------------------------------------------------------------------------------------------ the device steps
    def _device_steps(self, st):
        """Steps 2-7: everything between the frame upload and the record download, on the current stream, with no host
        synchronisation.  Returns the tensors whose memory the record was computed from (a capture keeps them)."""
        stream = torch.cuda.current_stream().cuda_stream
        K = self.K
        w = st.words.data_ptr()
        st.words.zero_()
        fmt, images = self._images(st)
        if self.tiles is None:
            call('cy_crop_resize_' + fmt, *images, st.frame_idx.data_ptr(), st.frame_rect.data_ptr(), st.n, self.side, self.side, 0.0, 1.0, 1,
                 st.x_dark.data_ptr(), w + 8, stream)
        else:               # every window of every frame, each resized as an image of its own
            call('cy_crop_resize_' + fmt, *images, st.tile_idx.data_ptr(), st.tile_rect.data_ptr(), st.n_dark, self.side, self.side, 0.0, 1.0, 1,
                 st.x_dark.data_ptr(), w + 8, stream)
        y = self.dark(st.x_dark).data
        if y.dim() != 4 or y.shape[0] != st.n_dark or y.shape[1] != self.g or y.shape[2] != self.g:
            raise ValueError('the detector returned %s for %d frames on a %d x %d grid' % (tuple(y.shape), st.n_dark, self.g, self.g))
        D = int(y.shape[3])
        nb = int((D - self.C) / 5)
        if nb < 1:          # what utils.decode_boxes_device refuses
            raise ValueError('y has %d values per cell: no box left after %d class scores (utils.py:291-293)' % (D, self.C))
        y = y.to(dtype=torch.float32).contiguous()
        if self.nms_iou is None:
            call('cy_yolo_decode_boxes_conf', y.data_ptr(), st.hw64.data_ptr(), float(self.side), float(self.side), st.n, self.g, nb, self.C,
                 self.conf_th, w, st.box_img.data_ptr(), st.box_xy.data_ptr(), st.box_cls.data_ptr() if self.C else None,
                 st.box_conf.data_ptr(), K, stream)
        elif self.tiles is not None:
            # the boxes of all windows in frame pixels into one candidate list per call (a frame's windows are neighbours in it), then
            # the suppression step per FRAME, which merges what the overlaps saw twice
            per_image = self.tiles.check_capacity(self.g, nb, query('cy_nms_max_per_image'))
            if st.cand is None or st.cand.cap != st.n * per_image:
                st.cand = _Candidates(st.n * per_image, st.n, K, self.C > 0, self.dev, tiled=True)
            c = st.cand
            c.words.zero_()
            cw = c.words.data_ptr()
            tw = cw + 4 * (2 + st.n)                     # dropped by the border rule, bad tiles (none: the table is tile_rects')
            call('cy_yolo_decode_tiles_conf', y.data_ptr(), st.tile_idx.data_ptr(), st.tile_rect.data_ptr(), st.hw32.data_ptr(), st.n,
                 self.tiles.margin, st.n_dark, self.g, nb, self.C, self.conf_th, cw, tw, c.img.data_ptr(), c.xy.data_ptr(),
                 c.cls.data_ptr() if self.C else None, c.conf.data_ptr(), None, c.cap, tw + 4, stream)
            call('cy_nms_boxes', cw, c.img.data_ptr(), c.xy.data_ptr(), c.conf.data_ptr(), c.cls.data_ptr() if self.C else None, c.cap,
                 st.n, self.nms_iou, int(self.nms_class_aware), self.per_frame, per_image, c.keep.data_ptr(), K, st.box_img.data_ptr(),
                 st.box_xy.data_ptr(), st.box_conf.data_ptr(), st.box_cls.data_ptr() if self.C else None, c.src.data_ptr(), w, cw + 8,
                 cw + 4, stream)
        else:
            # every box over the threshold into the candidate list, the survivors into the K slots, their number into the count word
            per_image = self.g * self.g * nb
            if st.cand is None or st.cand.cap != st.n * per_image:          # (first use: the eager pass in front of a capture)
                st.cand = _Candidates(st.n * per_image, st.n, K, self.C > 0, self.dev)
            c = st.cand
            c.words.zero_()
            cw = c.words.data_ptr()
            call('cy_yolo_decode_boxes_conf', y.data_ptr(), st.hw64.data_ptr(), float(self.side), float(self.side), st.n, self.g, nb, self.C,
                 self.conf_th, cw, c.img.data_ptr(), c.xy.data_ptr(), c.cls.data_ptr() if self.C else None, c.conf.data_ptr(), c.cap,
                 stream)
            # (the error word cannot fire: an image has at most per_image candidates, and that is the capacity asked for)
            call('cy_nms_boxes', cw, c.img.data_ptr(), c.xy.data_ptr(), c.conf.data_ptr(), c.cls.data_ptr() if self.C else None, c.cap,
                 st.n, self.nms_iou, int(self.nms_class_aware), self.per_frame, per_image, c.keep.data_ptr(), K, st.box_img.data_ptr(),
                 st.box_xy.data_ptr(), st.box_conf.data_ptr(), st.box_cls.data_ptr() if self.C else None, c.src.data_ptr(), w, cw + 8,
                 cw + 4, stream)
        call('cy_boxes_crop_resize_' + fmt, *images, w, st.box_img.data_ptr(), st.box_xy.data_ptr(), K, self.ci, self.ci, -128.0,
             1.0 / 128.0, 1, st.crops.data_ptr(), st.rect.data_ptr(), w + 4, stream)
        scores = self.cls(st.crops).data.reshape(K, -1).to(dtype=torch.float32).contiguous()
        call('cy_pack_detections', scores.data_ptr(), int(scores.shape[1]), w, st.box_img.data_ptr(), st.box_xy.data_ptr(),
             st.box_conf.data_ptr(), st.rect.data_ptr(), w + 4, w + 8, K, st.record.data_ptr(), stream)
        if self.tracker is not None:
            if int(scores.shape[1]) != self.tracker.n_classes:
                raise ValueError('the classifier returned %d scores per crop, the tracker was built for %d' % (scores.shape[1], self.tracker.n_classes))
            self.tracker.launch(w, st.box_xy.data_ptr(), st.box_conf.data_ptr(), st.rect.data_ptr(), scores.data_ptr(), stream)
        return y, scores

    def _weights_key(self):
        # the capture holds the folded eval weights (ops.fold_eval_bn): they are stale once ops' parameter epoch or a tensor's
        # version counter has moved (load_state_dict, an optimizer step, a switch of mode)
        return (ops.PARAM_EPOCH,) + tuple(t._version for t in self._tensors)

    def _capture(self, st):
        """GraphedStep's recipe: one eager pass on a side stream (fold caches, one-time kernel attributes, MIOpen's choices exist
        before the capture begins), then steps 2-7 captured on one stream.  The eager pass must not count as a frame: the tracker's
        state is put back behind it."""
        st.graph, st.keep = None, None
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            tracks = None if self.tracker is None else self.tracker.state.clone()
            self._device_steps(st)
            if tracks is not None:
                self.tracker.state.copy_(tracks)
        torch.cuda.current_stream(self.dev).wait_stream(side)
        torch.cuda.synchronize(self.dev)
        graph = torch.cuda.CUDAGraph()
        # torch.cuda.graph no longer collects on entry, and a dead cycle that holds a pinned buffer or an event (a detector that
        # raised: exception -> traceback -> frame -> state) must not be finalised while the stream captures: the frees record and
        # query events, which a capture refuses, and the error is thrown inside a destructor
        gc.collect()
        with torch.cuda.graph(graph):
            st.keep = self._device_steps(st)
        st.graph, st.graph_key = graph, self._weights_key()

    # ------------------------------------------------------------------------------------------------ the call
    def detect(self, frames, layout=None):
        on_dev, arrs, H, W, layout = self._sources(frames, layout)
        if self.tracker is not None and len(arrs) != 1:
            raise ValueError('a tracker follows one camera: one frame per call, got %d' % len(arrs))
        st = self._state(len(arrs), H, W, layout)
        if self.dark.training or self.cls.training:
            self.dark.eval()
            self.cls.eval()
        with torch.no_grad():
            if on_dev:
                # device to device on the current stream, in front of the steps (or the replay) that read the state's buffer
                fb = st.frame_bytes
                for k, t in enumerate(arrs):
                    st.frames[k * fb:(k + 1) * fb].copy_(t.reshape(-1), non_blocking=True)
            else:
                # the staging buffer is free: the previous call on this state waited for its record, which is behind its upload
                rows = st.stage()
                for k, a in enumerate(arrs):
                    np.copyto(rows[k].reshape(a.shape), a)
                st.frames.copy_(st.staging, non_blocking=True)
            if self.use_graph:
                if st.graph is None or st.graph_key != self._weights_key():
                    self._capture(st)
                st.graph.replay()
            else:
                self._device_steps(st)
            st.record_host.copy_(st.record, non_blocking=True)
            if self.tracker is not None:
                self.tracker.record_host.copy_(self.tracker.record, non_blocking=True)
            st.done.record(torch.cuda.current_stream(self.dev))
        st.done.synchronize()
        res = Detections(st.record_host.numpy().copy(), self.K)
        if self.tracker is not None:
            res.tracks = self.tracker.tracks()
        return res
