"""VideoDetector.detect_streams(heatmap=...): the heat maps of every camera accumulate on the device inside the step; between the
yields stream_heatmaps() equals host HeatMaps fed the yielded rows, and the yielded rows are those of a run without the option."""
import numpy as np
import pytest

from yolo_deepsort_amd import cfgs, heatmap as H, synth

pytestmark = pytest.mark.gpu
DS = dict(max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)


def test_detect_streams_accumulates_each_cameras_heat_map(tmp_path):
    """Two in-memory clips of different sizes (480 x 640 and 270 x 480, mixed_sizes=True), skip_frames=2, one HeatSpec per camera:
    after every step stream_heatmaps() holds, per stream, the layers of a host HeatMap fed that stream's processed, non-None rows
    with times frame index / 25."""
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import DeepSort
    from yolo_deepsort_amd.detect import VideoDetector
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=4, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0, -1.45))      # a handful of (random) detections per frame
    base = DeepSort(synth.reid_state_dict(0), use_cuda=True, **DS)
    clips = []
    for seed, n, hw in ((21, 13, (480, 640)), (22, 9, (270, 480))):
        img = np.random.RandomState(seed).randint(0, 256, hw + (3,)).astype(np.uint8)
        clips.append([np.roll(img, 3 * t, axis=1) for t in range(n)])
    specs = [H.HeatSpec(480, 640, 32, -1), H.HeatSpec(270, 480, 16, -1)]
    names = tmp_path / "coco.names"
    names.write_text(cfgs.coco_names_text())

    def detector():
        return VideoDetector(net, str(names), thres=0.5, nms_thres=0.4, tracker=base, skip_frames=2, class_mask=list(range(0, 80, 2)))
    plain = [[(s, det) for s, _, det, _ in step] for step in detector().detect_streams(clips, frames_per_stream=1, show_fps=False, mixed_sizes=True)]
    vd = detector()
    with pytest.raises(ValueError, match="between the yields"):
        vd.stream_heatmaps()
    hosts = [H.HeatMap(sp, max_age=3) for sp in specs]
    seen, items, counted = [0, 0], [], 0
    for step in vd.detect_streams(clips, frames_per_stream=1, show_fps=False, mixed_sizes=True, heatmap=specs, heatmap_max_age=3):
        for s, _, det, _ in step:
            if seen[s] % 2 == 0:                                      # a processed frame
                counted += hosts[s].update(det, seen[s] / 25.0) or 0
            seen[s] += 1
        got = vd.stream_heatmaps()
        assert all(np.array_equal(got[s], hosts[s].layer("presence")) for s in range(2))
        assert np.array_equal(vd.stream_heatmaps(layer=None, stream=1), hosts[1].layers())
        assert np.array_equal(vd.stream_heatmaps("dwell_us", 0), hosts[0].layer("dwell_us"))
        items.append([(s, det) for s, _, det, _ in step])
    assert seen == [13, 9] and counted >= 4 and sum(h.stats["dwell_credits"] for h in hosts) >= 2
    assert len(items) == len(plain)
    for a, b in zip(items, plain):
        assert [s for s, _ in a] == [s for s, _ in b]
        assert all((x is None) == (y is None) and (x is None or np.array_equal(x, y)) for (_, x), (_, y) in zip(a, b))
    with pytest.raises(ValueError, match="heatmap"):
        next(detector().detect_streams(clips, mixed_sizes=True, heatmap=[specs[0]]))
    with pytest.raises(ValueError, match="heatmap="):
        vd2 = detector()
        for _ in vd2.detect_streams(clips, frames_per_stream=1, show_fps=False, mixed_sizes=True):
            vd2.stream_heatmaps()
