"""GPU tests of the NV12 path: `cy_nv12_to_rgb_u8` against the numpy restatement of the colour rule (tests/nv12_ref.py), and every
other NV12 entry point -- the two crop launches, serve.SignDetector(frame_format='nv12'), device-resident frames, the command line --
against the existing RGB entry point run on the frame converted by that restatement, bit for bit.  No tolerance anywhere."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from helpers import REPO, make_params

import nv12_ref as R
import serve_ref
from capsyolo_amd import _lib, models, nv12, predict_fns, serve, synth, utils
from capsyolo_amd._lib import call
from capsyolo_amd.tiles import TileSpec

pytestmark = pytest.mark.gpu


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Packed(object):
    """NV12 surfaces (buf, H, W, pitch, uv_off) behind one another in one device buffer, with a gap of 3 bytes between them (no
    alignment is promised), and what the restatement makes of each."""

    def __init__(self, surfaces, matrix='bt601'):
        offs, parts, at = [], [], 0
        for buf, H, W, pitch, uv_off in surfaces:
            offs.append(at)
            parts += [buf, np.full(3, 0xEE, np.uint8)]
            at += buf.size + 3
        self.host = np.concatenate(parts)
        self.n, self.nbytes = len(surfaces), int(self.host.size)
        self.geom_host = [(H, W, pitch, uv_off) for _, H, W, pitch, uv_off in surfaces]
        self.off_host = offs
        self.buf, self.off, self.geom = _dev(self.host, np.uint8), _dev(offs, np.int64), _dev(self.geom_host, np.int32)
        self.rgb = [R.to_rgb(self.host, H, W, pitch, uv_off, matrix, o) for (H, W, pitch, uv_off), o in zip(self.geom_host, offs)]


def _surface(rng, H, W, pitch=None, uv_off=None):
    p, _ = R.tight(H, W)
    pitch = p if pitch is None else pitch
    uv_off = H * pitch if uv_off is None else uv_off
    return R.random_frame(rng, H, W, pitch, uv_off), H, W, pitch, uv_off


def _grid_surface():
    """Every triple of Y in {0, 15, 16, 17, 128, 235, 255} x U, V in {0, 1, 127, 128, 129, 255}: chroma block row i holds pair i,
    block column j holds luma j."""
    ys, cs = [0, 15, 16, 17, 128, 235, 255], [0, 1, 127, 128, 129, 255]
    H, W = 2 * len(cs) ** 2, 2 * len(ys)
    buf = np.zeros(R.nbytes(H, W), np.uint8)
    buf[:H * W].reshape(H, W)[:] = np.repeat(ys, 2)[None, :]
    uv = buf[H * W:].reshape(H // 2, W // 2, 2)
    uv[:, :, 0] = np.repeat(cs, len(cs))[:, None]
    uv[:, :, 1] = np.tile(cs, len(cs))[:, None]
    return buf, H, W, W, H * W


def _test_surfaces():
    rng = np.random.default_rng(12)
    return [_surface(rng, 2, 2), _surface(rng, 7, 9), _surface(rng, 8, 10, pitch=16), _surface(rng, 80, 100, uv_off=(80 + 8) * 100),
            _grid_surface()]


# ------------------------------------------------------------------------------------------------ 1. the whole-image conversion
@pytest.mark.parametrize('matrix', sorted(R.MATRICES))
def test_to_rgb_equals_the_restatement(matrix):
    p = _Packed(_test_surfaces(), matrix)
    sizes = [h * w * 3 for h, w, _, _ in p.geom_host]
    out_off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    out = torch.full((int(sum(sizes)),), 0xAB, dtype=torch.uint8, device='cuda')
    err = torch.zeros(1, dtype=torch.int32, device='cuda')
    d_out_off = _dev(out_off, np.int64)
    call('cy_nv12_to_rgb_u8', p.buf.data_ptr(), p.off.data_ptr(), p.geom.data_ptr(), p.n, p.nbytes, _lib.YuvCoef(*R.MATRICES[matrix]),
         out.data_ptr(), d_out_off.data_ptr(), out.numel(), err.data_ptr(), _stream())
    got = out.cpu().numpy()
    assert int(err.item()) == 0
    for k, (o, s) in enumerate(zip(out_off, sizes)):
        np.testing.assert_array_equal(got[o:o + s].reshape(p.rgb[k].shape), p.rgb[k], err_msg='surface %d' % k)
    # the grid surface makes values below 0 and over 255 occur in front of the clamp
    gbuf, H, W, pitch, uv_off = _grid_surface()
    pre, _ = R.before_clamp(*R.planes(gbuf, H, W), matrix=matrix)
    assert (pre < 0).any() and (pre > 255).any() and len(np.unique(np.stack(R.planes(gbuf, H, W), -1).reshape(-1, 3), axis=0)) == 7 * 36
    # the python wrapper: the same surfaces through nv12.to_rgb_device
    lays = [nv12.Layout(*g) for g in p.geom_host]
    views = nv12.to_rgb_device(p.buf, lays, matrix if matrix != 'bt709' else R.MATRICES['bt709'], offsets=p.off_host)
    for v, want in zip(views, p.rgb):
        np.testing.assert_array_equal(v.cpu().numpy(), want)


def test_to_rgb_leaves_a_bad_surface_alone():
    rng = np.random.default_rng(3)
    p = _Packed([_surface(rng, 4, 6), _surface(rng, 4, 6), _surface(rng, 4, 6), _surface(rng, 4, 6), _surface(rng, 4, 6)])
    geom = np.array(p.geom_host, dtype=np.int32)
    off = np.array(p.off_host, dtype=np.int64)
    geom[0, 2] = 5                  # pitch shorter than a chroma row
    geom[1, 3] = 4 * 6 - 1          # the chroma plane begins inside the Y plane
    off[2] = -1                     # in front of the buffer
    off[4] = p.nbytes - 30          # the chroma plane ends behind the buffer
    out = torch.full((5 * 72,), 0xAB, dtype=torch.uint8, device='cuda')
    err = torch.zeros(1, dtype=torch.int32, device='cuda')
    d = [_dev(off, np.int64), _dev(geom, np.int32), _dev(np.arange(5) * 72, np.int64)]
    call('cy_nv12_to_rgb_u8', p.buf.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), 5, p.nbytes, _lib.YuvCoef(*R.MATRICES['bt601']),
         out.data_ptr(), d[2].data_ptr(), out.numel(), err.data_ptr(), _stream())
    got = out.cpu().numpy().reshape(5, 72)
    assert int(err.item()) == 4 and (got[[0, 1, 2, 4]] == 0xAB).all()
    np.testing.assert_array_equal(got[3].reshape(4, 6, 3), p.rgb[3])


# ------------------------------------------------------------------------------------------------ 2. crop + resize
RECTS = [(0, 0, 7, 0, 9),            # the whole odd-sized frame
         (1, 0, 80, 0, 100),         # the whole padded frame
         (1, 11, 50, 23, 70),        # odd y0 and x0
         (0, 6, 7, 7, 8),            # 1 x 1 in the last row at an odd column
         (0, 5, 6, 8, 9),            # 1 x 1 in the last column at an odd row
         (0, 6, 7, 8, 9),            # 1 x 1, the last pixel: the half-empty chroma block
         (0, 1, 4, 3, 5),            # 3 x 2, upscaled
         (1, 10, 90, 0, 10),         # bad: leaves the frame
         (2, 0, 1, 0, 1)]            # bad: no such image
N_BAD = 2


def _crop_pair():
    rng = np.random.default_rng(21)
    p = _Packed([_surface(rng, 7, 9, pitch=13, uv_off=7 * 13 + 5), _surface(rng, 80, 100, pitch=112, uv_off=96 * 112)])
    return p, predict_fns.PackedImages(p.rgb)


@pytest.mark.parametrize('side', [5, 32])
@pytest.mark.parametrize('to_nchw', [False, True])
@pytest.mark.parametrize('shift,scale', [(0.0, 1.0), (-128.0, 1.0 / 128.0)])
def test_crop_resize_equals_the_rgb_entry_point_bit_for_bit(side, to_nchw, shift, scale):
    p, packed = _crop_pair()
    idx, rect = _dev([r[0] for r in RECTS], np.int32), _dev([r[1:] for r in RECTS], np.int32)
    n = len(RECTS)
    shape = (n, 3, side, side) if to_nchw else (n, side, side, 3)
    outs, errs = [], []
    for fmt in ('nv12', 'u8'):
        out = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
        err = torch.zeros(1, dtype=torch.int32, device='cuda')
        if fmt == 'nv12':
            head = (p.buf.data_ptr(), p.off.data_ptr(), p.geom.data_ptr(), p.n, p.nbytes, _lib.YuvCoef(*R.MATRICES['bt601']))
        else:
            head = (packed.buf.data_ptr(), packed.off.data_ptr(), packed.hw32.data_ptr(), packed.n, packed.nbytes)
        call('cy_crop_resize_' + fmt, *head, idx.data_ptr(), rect.data_ptr(), n, side, side, float(shift), float(scale), int(to_nchw),
             out.data_ptr(), err.data_ptr(), _stream())
        outs.append(out.cpu().numpy())
        errs.append(int(err.item()))
    assert errs == [N_BAD, N_BAD]
    assert outs[0].tobytes() == outs[1].tobytes()
    assert not np.isnan(outs[0]).any() and not outs[0][-N_BAD:].any()
    flat = outs[0].reshape(n, -1)
    assert all(np.unique(flat[k]).size > 1 for k in (0, 1, 2, 6))        # real pictures, not constants
    px = (p.rgb[0][6, 8].astype(np.float32) + np.float32(shift)) * np.float32(scale)       # a 1 x 1 crop is its pixel everywhere
    got = outs[0][5].reshape(3, -1).T if to_nchw else outs[0][5].reshape(-1, 3)
    assert (got == px[None, :]).all()


# ------------------------------------------------------------------------------------------------ 3. the box crops
BOX_IDX = np.array([1, 1, 1, 0, 1, 1, 2, 1])
BOX_XY = np.array([[23.3, 11.7, 70.9, 50.2],         # interior, odd corner
                   [-3.5, -2.2, 36.8, 25.1],         # hangs over the left / top border: clipped
                   [61.1, 48.4, 125.0, 130.0],       # hangs over the right / bottom border
                   [8.2, 6.1, 9.9, 7.5],             # one pixel, the last of the odd-sized frame
                   [4.2, 5.0, 4.9, 8.0],             # empty after truncation
                   [1.0, np.nan, 5.0, 5.0],          # a corner that is not a number
                   [1.0, 1.0, 5.0, 5.0],             # no such image
                   [3.0, 2.0, 9.0, 7.0]])            # live only when the count says so
BOX_BAD = [4, 5, 6]


@pytest.mark.parametrize('side', [5, 32])
@pytest.mark.parametrize('to_nchw', [False, True])
@pytest.mark.parametrize('shift,scale', [(0.0, 1.0), (-128.0, 1.0 / 128.0)])
def test_boxes_crop_equals_the_rgb_entry_point_bit_for_bit(side, to_nchw, shift, scale):
    p, packed = _crop_pair()
    K = 8
    bi, bxy = _dev(BOX_IDX, np.int32), _dev(BOX_XY, np.float64)
    shape = (K, 3, side, side) if to_nchw else (K, side, side, 3)
    for count in (7, 20, 0):
        live = min(count, K)
        got = []
        for fmt in ('nv12', 'u8'):
            words = _dev([count, 0], np.int32)
            out = torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
            rect = torch.full((K, 4), -7, dtype=torch.int32, device='cuda')
            if fmt == 'nv12':
                head = (p.buf.data_ptr(), p.off.data_ptr(), p.geom.data_ptr(), p.n, p.nbytes, _lib.YuvCoef(*R.MATRICES['bt601']))
            else:
                head = (packed.buf.data_ptr(), packed.off.data_ptr(), packed.hw32.data_ptr(), packed.n, packed.nbytes)
            call('cy_boxes_crop_resize_' + fmt, *head, words.data_ptr(), bi.data_ptr(), bxy.data_ptr(), K, side, side, float(shift),
                 float(scale), int(to_nchw), out.data_ptr(), rect.data_ptr(), words.data_ptr() + 4, _stream())
            got.append((out.cpu().numpy(), rect.cpu().numpy(), int(words[1].item())))
        (out, rect, err), (out_u8, rect_u8, err_u8) = got
        assert out.tobytes() == out_u8.tobytes() and np.array_equal(rect, rect_u8) and err == err_u8
        ref_rect, ref_bad, ref_live = serve_ref.slot_rectangles(count, BOX_IDX, BOX_XY, [(7, 9), (80, 100)], K)
        assert np.array_equal(rect, ref_rect) and err == int(ref_bad.sum()) == len([s for s in BOX_BAD if s < live])
        rest = [s for s in range(K) if s >= live or s in BOX_BAD]         # bad and dead slots: exactly zero, zero rectangle
        assert not out[rest].any() and not np.isnan(out).any() and not rect[rest].any()
        good = [s for s in range(live) if s not in BOX_BAD]
        assert all(rect[s].any() for s in good)
        if count == 7:
            assert rect[0].tolist() == [11, 50, 23, 70] and rect[3].tolist() == [6, 7, 8, 9] and 7 in rest and out[0].any()


# ------------------------------------------------------------------------------------------------ 4 - 6. the detector
K_PIPE = 8
SEED = 41        # the RGB chain alone keeps two boxes and an odd rectangle corner on these frames (`_Chain.scenario` asserts it)


def _rgb_frames(seed, h=80, w=100, n=2):
    return [np.ascontiguousarray(im[:h, :w]) for im in synth.raw_images(n, seed=seed, min_side=max(h, w), max_side=160)]


class _Chain(object):
    """The small chain of tests/test_gpu_serve.py."""

    def __init__(self):
        self.dp = make_params(model='darknet_d', n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
        self.cp = make_params(model='capsule', n_classes=3, device='cuda')
        torch.manual_seed(3)
        self.dark, self.caps = models.DarkNet(self.dp).cuda().eval(), models.CapsuleNet(self.cp).cuda().eval()
        self.cache = {}

    def detector(self, conf_th, **kw):
        return serve.SignDetector(self.dark, self.dp, self.caps, self.cp, max_boxes=K_PIPE, conf_th=conf_th, **kw)

    def threshold(self, rgb):
        """Between the 5th and the 6th of the detector's confidences on these frames."""
        with torch.no_grad():
            y = self.dark(predict_fns.PackedImages(rgb).resize(64, to_nchw=True)).data
        conf = np.unique(y[..., 0::5].cpu().numpy())[::-1].astype(np.float64)
        assert len(conf) >= 7, 'the detector output has too few distinct confidences: %s' % conf
        return float(conf[4] + conf[5]) / 2

    def scenario(self, name, per_call, make_kw):
        """The frames of seed SEED (four, `per_call` of them per call), the threshold, and what the RGB chain ALONE makes of the frames
        converted by the restatement.  The comparison must not be empty: that chain keeps >= 2 boxes in some record, none bad, and a
        kept rectangle has an odd x0 or y0 -- asserted here, for this seed.
        Returns (conf_th, the calls' NV12 frames, the restatement's RGB frames, the RGB detector's results)."""
        if name in self.cache:
            return self.cache[name]
        four = _rgb_frames(SEED) + _rgb_frames(SEED + 100)
        f_nv12 = [nv12.from_rgb(f) for f in four]
        f_rgb = [R.to_rgb(f) for f in f_nv12]
        calls = [list(range(k, k + per_call)) for k in range(0, 4, per_call)]
        th = self.threshold([f_rgb[i] for i in calls[0]])
        det = self.detector(th, **make_kw())
        res = [det.detect([f_rgb[i] for i in c]) for c in calls]
        rects = [serve_ref.slot_rectangles(r.n, r.image_indices, r.boxes_xy, [(80, 100)] * per_call, K_PIPE)[0][:r.n] for r in res]
        odd = any((rc[:, 0] % 2 == 1).any() or (rc[:, 2] % 2 == 1).any() for rc in rects if len(rc))
        print('%s: seed %d keeps %s boxes, odd corner: %s' % (name, SEED, [r.n for r in res], odd))
        assert max(r.n for r in res) >= 2 and odd and all(r.bad == {'boxes': 0, 'frames': 0} for r in res)
        self.cache[name] = (th, [[f_nv12[i] for i in c] for c in calls], [[f_rgb[i] for i in c] for c in calls], res)
        return self.cache[name]


@pytest.fixture(scope='module')
def chain():
    return _Chain()


@pytest.fixture(scope='module')
def plain(chain):
    return chain.scenario('plain', 2, dict)


def test_detector_on_nv12_equals_the_detector_on_the_converted_frames(chain, plain):
    th, f_nv12, f_rgb, want = plain
    assert max(r.n for r in want) >= 2                                   # (the scenario's condition, asserted where it is used)
    det = chain.detector(th, frame_format='nv12')
    for frames, w in zip(f_nv12, want):
        res = det.detect(frames)
        assert res.record.tobytes() == w.record.tobytes()
        again = det.detect(np.stack(frames))                             # an [n, H + H/2, W] array; the same state
        assert again.record.tobytes() == w.record.tobytes()
    assert list(det.states) == [(2, nv12.Layout(80, 100))]
    assert not np.array_equal(want[0].record, want[1].record)
    # another table gives another picture, so in general another record; the same table as six integers gives the same
    same = chain.detector(th, frame_format='nv12', yuv_matrix=R.MATRICES['bt601']).detect(f_nv12[0])
    assert same.record.tobytes() == want[0].record.tobytes()
    other = chain.detector(th, frame_format='nv12', yuv_matrix='bt709_full').detect(f_nv12[0])
    full = chain.detector(th).detect([R.to_rgb(f, matrix='bt709_full') for f in f_nv12[0]])
    assert other.record.tobytes() == full.record.tobytes()


def test_graph_replays_two_frame_pairs_through_one_capture(chain, plain):
    th, f_nv12, f_rgb, want = plain
    det = chain.detector(th, frame_format='nv12', graph=True)
    first = det.detect(f_nv12[0])
    state = det.states[(2, nv12.Layout(80, 100))]
    graph = state.graph
    assert graph is not None and first.record.tobytes() == want[0].record.tobytes()
    assert det.detect(f_nv12[1]).record.tobytes() == want[1].record.tobytes()
    assert det.detect(f_nv12[0]).record.tobytes() == want[0].record.tobytes()
    assert state.graph is graph and len(det.states) == 1
    rgb = chain.detector(th, graph=True)                                 # the RGB capture beside it: today's path, graphed
    assert rgb.detect(f_rgb[1]).record.tobytes() == want[1].record.tobytes()


def test_nms_and_tiles_on_nv12(chain):
    make = lambda: dict(nms_iou=0.45, tiles=TileSpec(1, 2, 16))
    th, f_nv12, f_rgb, want = chain.scenario('tiles', 2, make)
    assert max(r.n for r in want) >= 2
    det = chain.detector(th, frame_format='nv12', **make())
    for frames, w in zip(f_nv12, want):
        assert det.detect(frames).record.tobytes() == w.record.tobytes()


def test_tracker_over_four_nv12_frames(chain):
    make = lambda: dict(tracker=serve.SignTracker(3, K_PIPE))
    th, f_nv12, f_rgb, want = chain.scenario('track', 1, make)
    assert len(want) == 4 and max(r.n for r in want) >= 2
    det = chain.detector(th, frame_format='nv12', **make())
    for frames, w in zip(f_nv12, want):
        res = det.detect(frames)
        assert res.record.tobytes() == w.record.tobytes()
        assert res.tracks.record.tobytes() == w.tracks.record.tobytes()
        assert res.tracks.ids.tolist() == w.tracks.ids.tolist() and res.tracks.frame == w.tracks.frame
    assert want[-1].tracks.frame == 4 and want[-1].tracks.live >= 1


def test_padded_layout_gives_the_record_of_the_tight_one(chain, plain):
    th, f_nv12, f_rgb, want = plain
    lay = nv12.Layout(80, 100, pitch=100 + 12, uv_off=96 * 112)
    tight = [nv12.from_rgb(f) for f in f_rgb[0]]
    padded = [nv12.from_rgb(f, layout=lay) for f in f_rgb[0]]
    for f, g in zip(padded, tight):                                      # the same samples: only where they lie differs
        assert all(np.array_equal(a, b) for a, b in zip(R.planes(f, 80, 100, lay.pitch, lay.uv_off), R.planes(g, 80, 100)))
    det = chain.detector(th, frame_format='nv12')
    a = det.detect(tight)
    b = det.detect(padded, layout=lay)
    c = det.detect([f.reshape(-1, lay.pitch) for f in padded], layout=lay)         # the 2-D form of the same buffers
    assert a.record.tobytes() == b.record.tobytes() == c.record.tobytes() and a.n >= 1
    assert a.record.tobytes() == chain.detector(th).detect([R.to_rgb(f) for f in tight]).record.tobytes()
    assert sorted(det.states, key=repr) == sorted([(2, nv12.Layout(80, 100)), (2, lay)], key=repr)
    with pytest.raises(ValueError, match='bytes'):
        det.detect([f[:-1] for f in padded], layout=lay)
    with pytest.raises(ValueError, match='layout'):
        chain.detector(th).detect(f_rgb[0], layout=lay)


@pytest.mark.parametrize('graph', [False, True])
@pytest.mark.parametrize('fmt', ['rgb', 'nv12'])
def test_device_resident_frames_give_the_record_of_host_frames(chain, plain, fmt, graph):
    th, f_nv12, f_rgb, want = plain
    calls = f_rgb if fmt == 'rgb' else f_nv12
    det = chain.detector(th, frame_format=fmt, graph=graph)
    for frames, w in zip(calls, want):
        on_dev = [torch.from_numpy(f).cuda() for f in frames]
        keep = [t.clone() for t in on_dev]
        assert det.detect(on_dev).record.tobytes() == w.record.tobytes()
        assert det.detect(torch.stack(on_dev)).record.tobytes() == w.record.tobytes()
        assert all(torch.equal(a, b) for a, b in zip(on_dev, keep))
    state, = det.states.values()
    assert state.staging is None                                         # no staging buffer was ever built
    assert det.detect(calls[0]).record.tobytes() == want[0].record.tobytes() and state.staging is not None   # host frames, same state


@pytest.mark.parametrize('fmt', ['rgb', 'nv12'])
def test_device_resident_frames_refusals(chain, plain, fmt):
    th, f_nv12, f_rgb, want = plain
    frames = (f_rgb if fmt == 'rgb' else f_nv12)[0]
    det = chain.detector(th, frame_format=fmt)
    good = torch.from_numpy(frames[0]).cuda()
    with pytest.raises(ValueError, match='is a tensor on cpu, the detector is on cuda'):
        det.detect(torch.from_numpy(frames[0]))
    with pytest.raises(ValueError, match='expected a torch.uint8 tensor, got dtype torch.float32'):
        det.detect(good.float())
    with pytest.raises(ValueError, match='not contiguous'):
        det.detect(torch.stack([good, good], dim=1)[:, 0])
    with pytest.raises(ValueError, match='host arrays and device tensors mixed'):
        det.detect([good, frames[1]])
    with pytest.raises(ValueError, match='one size'):
        det.detect([good, good[:-6, :-2].contiguous()] if fmt == 'nv12' else [good, good[:, :90].contiguous()])
    assert not det.states                                                # nothing was built for a refused call


# ------------------------------------------------------------------------------------------------ 7. the command line
def test_main_serve_mode_with_nv12_device_frames(tmp_path):
    dp = make_params(model='darknet_d', n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, device='cuda')
    cp = make_params(model='capsule', n_classes=43, device='cuda')
    torch.manual_seed(3)
    ddir, cdir = str(tmp_path / 'darknet_d'), str(tmp_path / 'capsule')
    utils.save_checkpoint({'epoch': 0, 'state_dict': models.DarkNet(dp).state_dict()}, False, ddir)
    utils.save_checkpoint({'epoch': 0, 'state_dict': models.CapsuleNet(cp).state_dict()}, False, cdir)
    json.dump(dict(batch_size=4, n_classes=0, n_grid=2, n_boxes=2, darknet_input=64, capsule_input=32, dropout=0.0),
              open(os.path.join(ddir, 'params.json'), 'w'))
    json.dump(dict(batch_size=8, n_classes=43), open(os.path.join(cdir, 'params.json'), 'w'))
    spec = importlib.util.spec_from_file_location('cy_main_serve_nv12', os.path.join(REPO, 'main.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = m.main(['--mode', 'serve', '--model', 'darknet_d', '--combine', 'capsule', '--synthetic', '3', '--model_dir', ddir,
                  '--restore', 'last', '--frame_format', 'nv12', '--device_frames'])
    lines = open(os.path.join(ddir, 'serve_output.txt')).read().splitlines()
    assert len(lines) == 3 and [ln.split(':')[0] for ln in lines] == ['frame 0', 'frame 1', 'frame 2']
    assert out['frames'] == 3 and out['boxes'] == sum(int(ln.split('boxes: ')[1].split(' of ')[0]) for ln in lines)
    sizes = [tuple(int(v) for v in ln.split(': ')[1].split(' |')[0].split('x')) for ln in lines]
    raw = [f.shape[:2] for f in synth.raw_images(3)]
    assert sizes == [(h - h % 2, w - w % 2) for h, w in raw]             # the line says the size used
