"""Host side of the per-stream window setting (MultiStreamPipeline(stream_win_sizes=...), VideoDetector.detect_streams(stream_win_sizes=...)):
the argument checks that run before any device call."""
import numpy as np
import pytest

from yolo_deepsort_amd import cfgs
from yolo_deepsort_amd import detect as D
from yolo_deepsort_amd import pipeline as pl


def test_check_stream_win_sizes():
    assert pl.check_stream_win_sizes(3, None, None) is None
    assert pl.check_stream_win_sizes(3, (416, 416), None) is None
    assert pl.check_stream_win_sizes(3, None, [(416, 416), None, [320.0, 240]]) == [(416, 416), None, (320, 240)]
    with pytest.raises(ValueError, match="exclude"):                  # one setting for all streams, or one per stream
        pl.check_stream_win_sizes(2, (416, 416), [None, None])
    with pytest.raises(ValueError, match=r"one entry per stream \(2\), got 3"):
        pl.check_stream_win_sizes(2, None, [None, None, None])
    for bad in ((416,), (416, 0), (-1, 416), (1, 2, 3)):
        with pytest.raises(ValueError, match=r"stream_win_sizes\[1\]"):
            pl.check_stream_win_sizes(2, None, [None, bad])


def test_multi_stream_pipeline_checks_its_arguments_before_the_device():
    """Neither call reaches the library: the stand-ins for the detector and the DeepSort objects have nothing to hand to it."""
    with pytest.raises(ValueError, match="exclude"):
        pl.MultiStreamPipeline(None, [object(), object()], win_size=(416, 416), stream_win_sizes=[(416, 416), None])
    with pytest.raises(ValueError, match="one entry per stream"):
        pl.MultiStreamPipeline(None, [object(), object()], stream_win_sizes=[(416, 416)])


def test_detect_streams_checks_stream_win_sizes_first(tmp_path):
    class Model:
        img_size = (416, 416)
        batch_max = 4

        def eval(self):
            return self

        def parameters(self):
            yield type("P", (), {"device": "cpu"})()

    names = tmp_path / "coco.names"
    names.write_text(cfgs.coco_names_text())
    a = np.zeros((96, 128, 3), np.uint8)
    vd = D.VideoDetector(Model(), str(names), tracker=None)
    with pytest.raises(ValueError, match="one entry per stream"):
        list(vd.detect_streams([[a], [a]], show_fps=False, stream_win_sizes=[(64, 64)]))
    with pytest.raises(ValueError, match="tracker"):                  # a well-formed list: the next check speaks
        list(vd.detect_streams([[a], [a]], show_fps=False, stream_win_sizes=[(64, 64), None]))
    vd = D.VideoDetector(Model(), str(names), tracker=None, win_size=(64, 64))
    with pytest.raises(ValueError, match="win_size"):                 # the detector's own win_size and one per stream: one or the other
        list(vd.detect_streams([[a], [a]], show_fps=False, stream_win_sizes=[(64, 64), None]))
