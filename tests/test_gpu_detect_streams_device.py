"""VideoDetector.detect_streams with the output stage on the device (staged uploads, look-ahead, DeviceOverlay.render /
render_mixed over the staged block) against the same call with device_overlay=False - today's host loop: every yielded list equal
(stream indices and order, image shapes and bytes, rows, actions), and everything read between the yields equal, which is the
lock-step condition of the device form."""
import functools
import threading

import numpy as np
import pytest

from yolo_deepsort_amd import cfgs, synth
from yolo_deepsort_amd.privacy import Anonymize

pytestmark = pytest.mark.gpu
DS = dict(max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)
IMG = (416, 416)


@functools.lru_cache(maxsize=None)
def _net(obj_bias=-1.45, batch_max=8):
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    cfg = cfgs.cfg_text("yolov3-tiny", *IMG)
    net = Darknet(None, img_size=IMG, batch_max=batch_max, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0, obj_bias))      # a handful of (random) detections per frame
    return net


@functools.lru_cache(maxsize=None)
def _base():
    from yolo_deepsort_amd.deep_sort import DeepSort
    _net()
    return DeepSort(synth.reid_state_dict(0), use_cuda=True, **DS)


def _detector(tmp_path, device, **kw):
    from yolo_deepsort_amd.detect import VideoDetector
    names = tmp_path / "coco.names"
    names.write_text(cfgs.coco_names_text())
    kw.setdefault("class_mask", list(range(0, 80, 2)))
    net = _net(*kw.pop("net", ()))
    return VideoDetector(net, str(names), thres=0.5, nms_thres=0.4, tracker=_base().clone(), device_overlay=device, **kw)


def _clips(sizes, lengths, seed=21):
    clips = []
    for k, ((h, w), n) in enumerate(zip(sizes, lengths)):
        base = np.random.RandomState(seed + k).randint(0, 256, (h, w, 3)).astype(np.uint8)
        clips.append([np.roll(base, 3 * t, axis=1) for t in range(n)])
    return clips


def _run(tmp_path, device, clips, det_kw, call_kw, between=None):
    vd = _detector(tmp_path, device, **det_kw)
    assert vd.device_overlay == device
    steps, reads = [], []
    for step in vd.detect_streams(clips, show_fps=False, **call_kw):
        steps.append([(s, img.copy(), None if det is None else np.array(det, np.int32).reshape(-1, 6), list(act)) for s, img, det, act in step])
        if between is not None:
            reads.append(between(vd))
    assert getattr(vd, "_streams_pipe", None) is None
    return steps, reads, vd


def _assert_equal_steps(a, b):
    assert len(a) == len(b)
    rows = 0
    for k, (x, y) in enumerate(zip(a, b)):
        assert [s for s, *_ in x] == [s for s, *_ in y], k
        for (s, img, det, act), (_, wimg, wdet, wact) in zip(x, y):
            assert img.shape == wimg.shape and img.dtype == np.uint8, (k, s)
            assert (det is None) == (wdet is None) and (det is None or np.array_equal(det, wdet)), (k, s)
            assert act == wact, (k, s)
            assert np.array_equal(img, wimg), (k, s, int((img != wimg).any(-1).sum()))
            rows += 0 if det is None else len(det)
    return rows


UNIFORM, TWO = [(240, 320)] * 3, [(240, 320), (135, 250), (240, 320)]
CASES = {
    "uniform": (UNIFORM, [6, 6, 6], {}, dict(frames_per_stream=1)),
    "mixed": (TWO, [6, 6, 6], {}, dict(frames_per_stream=1, mixed_sizes=True)),
    "skip2": (TWO, [7, 7, 7], dict(skip_frames=2), dict(frames_per_stream=1, mixed_sizes=True)),
    "skip2-uniform": (UNIFORM, [7, 7, 7], dict(skip_frames=2), dict(frames_per_stream=1)),
    "two-per-stream": (TWO, [8, 8, 7], {}, dict(frames_per_stream=2, mixed_sizes=True)),
    "ends-early": (TWO, [8, 5, 8], {}, dict(frames_per_stream=1, mixed_sizes=True)),
    "ends-early-uniform": (UNIFORM, [8, 5, 8], {}, dict(frames_per_stream=1)),
    "pixelate": (TWO, [6, 6, 6], dict(anonymize=Anonymize(classes=None)), dict(frames_per_stream=1, mixed_sizes=True)),
    "fill": (UNIFORM, [6, 6, 6], dict(anonymize=Anonymize(mode="fill", color=(200, 30, 5), classes=None), skip_frames=2),
             dict(frames_per_stream=1)),
    "windows": ([(480, 640), (135, 250), (240, 320)], [5, 5, 5], dict(net=(-1.3, 4), class_mask=None),
                dict(frames_per_stream=1, mixed_sizes=True, stream_win_sizes=[(416, 416), None, None])),
}


@pytest.mark.parametrize("case", list(CASES))
def test_device_form_yields_what_the_host_form_yields(tmp_path, case):
    sizes, lengths, det_kw, call_kw = CASES[case]
    clips = _clips(sizes, lengths, seed=40 if case == "windows" else 21)
    host, _, _ = _run(tmp_path, False, clips, det_kw, call_kw)
    dev, _, vd = _run(tmp_path, True, clips, det_kw, call_kw)
    assert _assert_equal_steps(dev, host) > 0
    ahead, steps = vd.streams_lookahead
    assert 0 < steps <= len(host)
    if case in ("uniform", "mixed"):
        assert ahead == steps - 1                       # files are read ahead: every step but the last carries the next one's pass
    if case.startswith("ends-early"):
        assert 0 < ahead < steps - 1                    # the step before the composition changes passes None


def test_reads_between_the_yields_are_those_of_the_yielded_step(tmp_path):
    """Zone events and counts and the global ids, read after every yield: the device form steps in lock-step with its yields, so
    they are the host form's, step by step - with a look-ahead pass in flight."""
    from yolo_deepsort_amd import zones as Z
    clips = _clips(TWO, [8, 6, 8])
    zones = [Z.Zone([(10, 10), (200, 10), (200, 200), (10, 200)], name="left"), Z.Zone([(100, 50), (300, 50), (300, 230), (100, 230)], name="mid")]
    lines = [Z.Line((0, 120), (320, 120), name="across"), Z.Line((125, 0), (125, 135), name="down")]
    call_kw = dict(frames_per_stream=1, mixed_sizes=True, zones=(zones, lines), zone_max_age=3)

    def between(vd):
        return vd.stream_zone_events(), vd.stream_zone_counts()
    host, host_reads, _ = _run(tmp_path, False, clips, {}, call_kw, between)
    dev, dev_reads, vd = _run(tmp_path, True, clips, {}, call_kw, between)
    assert _assert_equal_steps(dev, host) > 0
    assert vd.streams_lookahead[0] > 0
    assert len(dev_reads) == len(host_reads)
    for k, (a, b) in enumerate(zip(dev_reads, host_reads)):
        assert a == b, k
    # global ids: the map is the caller's to change between the yields, so such a run carries no look-ahead pass
    call_kw["global_ids"] = True

    def between_ids(vd):
        return vd.stream_zone_events(), vd.stream_zone_counts(), vd.stream_identities()
    host, host_reads, _ = _run(tmp_path, False, clips, {}, call_kw, between_ids)
    dev, dev_reads, vd = _run(tmp_path, True, clips, {}, call_kw, between_ids)
    assert _assert_equal_steps(dev, host) > 0 and dev_reads == host_reads
    assert vd.streams_lookahead[0] == 0 and vd.streams_lookahead[1] > 0
    assert any(ids for _, _, per in host_reads for ids in per)            # some track held a global id at some step


def test_identity_memory_runs_without_look_ahead(tmp_path):
    """The map of a run with identity_memory may be enrolled into between the yields, which the library refuses while a
    look-ahead pass is in flight: such a run carries none, and an enrol after the first yield goes through."""
    clips = _clips(UNIFORM, [4, 4, 4])
    vd = _detector(tmp_path, True)
    for k, _ in enumerate(vd.detect_streams(clips, frames_per_stream=1, show_fps=False, global_ids=True, identity_memory=dict(ids=4, rows=4))):
        if k == 0:
            row = np.zeros((1, 512), np.float32)
            row[0, 0] = 1.0
            assert len(vd.stream_identity_map().enrol([row])) == 1
    assert vd.streams_lookahead == [0, 4]


@pytest.mark.parametrize("mixed", [False, True])
def test_file_sources_are_staged_as_bgr_and_drawn_on_in_place(tmp_path, mixed):
    """Sources that are all files (.npy clips, BGR as a decoder delivers them): the device form stages the BGR, reads it in that
    order and draws in place (render(bgr_frames=...) / render_mixed(bgr=True)); the yields are the host form's, skip_frames and the
    anonymise option included."""
    sizes = TWO if mixed else UNIFORM
    paths = []
    for k, clip in enumerate(_clips(sizes, [6, 4, 6], seed=31)):
        paths.append(str(tmp_path / ("clip%d.npy" % k)))
        np.save(paths[-1], np.stack([f[:, :, ::-1] for f in clip], 0))
    for det_kw in (dict(skip_frames=2), dict(anonymize=Anonymize(classes=None))):
        call_kw = dict(frames_per_stream=1, mixed_sizes=mixed)
        host, _, _ = _run(tmp_path, False, paths, det_kw, call_kw)
        dev, _, vd = _run(tmp_path, True, paths, det_kw, call_kw)
        assert _assert_equal_steps(dev, host) > 0
        assert vd._streams_pipe is None and vd.streams_lookahead[0] > 0


def test_device_run_never_renders_on_the_host(tmp_path, monkeypatch):
    from yolo_deepsort_amd.detect import VideoDetector

    def boom(*a, **k):
        raise AssertionError("the host renderer ran")
    monkeypatch.setattr(VideoDetector, "_render_host", boom)
    for sizes, kw in ((UNIFORM, {}), (TWO, dict(mixed_sizes=True))):
        steps, _, _ = _run(tmp_path, True, _clips(sizes, [4, 4, 4]), dict(skip_frames=2), dict(frames_per_stream=1, **kw))
        assert sum(len(st) for st in steps) == 12             # (the last step holds skipped frames only: rendered, not stepped)


def test_closing_the_generator_joins_the_reader(tmp_path):
    vd = _detector(tmp_path, True)
    before = threading.active_count()
    gen = vd.detect_streams(_clips(TWO, [30, 30, 30]), frames_per_stream=1, show_fps=False, mixed_sizes=True)
    first = next(gen)
    assert len(first) == 3 and vd._streams_pipe is not None
    reader = vd._streams_reader
    assert reader.is_alive()
    gen.close()
    reader.join(timeout=5)
    assert not reader.is_alive() and vd._streams_pipe is None
    assert threading.active_count() <= before
    with pytest.raises(ValueError, match="between the yields"):
        vd.search_streams(np.zeros((1, 512), np.float32))


def test_a_source_that_raises_surfaces_on_the_callers_thread(tmp_path):
    class Broken(Exception):
        pass

    def source(n):
        for f in _clips([(240, 320)], [n])[0]:
            yield f
        raise Broken("camera 1 fell over")
    vd = _detector(tmp_path, True)
    got = []
    with pytest.raises(Broken, match="camera 1"):
        for step in vd.detect_streams([_clips([(240, 320)], [9])[0], source(3)], frames_per_stream=1, show_fps=False):
            got.append(len(step))
    assert got == [2, 2, 2] and vd._streams_pipe is None
    # a stream that changes its shape is refused with the stream named, as on the host form
    a, b = np.zeros((64, 80, 3), np.uint8), np.zeros((48, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="stream 1"):
        list(_detector(tmp_path, True).detect_streams([[a, a, a], [b, b, a]], frames_per_stream=1, show_fps=False, mixed_sizes=True))
