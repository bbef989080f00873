from yolo_deepsort_amd.detect import VideoDetector as _VideoDetector


class VideoDetector(_VideoDetector):
    """The drop-in at the reference's import path keeps the constructor that tests/test_host_logic.py pins (the reference's
    parameters, then batch_frames and device_overlay).  What yolo_deepsort_amd.detect.VideoDetector takes beyond it is an attribute
    here: ``vd.batch_windows = True``, ``vd.anonymize = privacy.Anonymize(...)``."""

    def __init__(self, model, class_path, thickness=2, font_path=None, font_size=10, thres=0.7, nms_thres=0.4,
                 skip_frames=-1, fourcc="mp4v", class_mask=None, win_size=None, overlap=0.15, tracker=None,
                 action_id=None, half=False, batch_frames=None, device_overlay=True):
        super().__init__(model, class_path, thickness=thickness, font_path=font_path, font_size=font_size, thres=thres,
                         nms_thres=nms_thres, skip_frames=skip_frames, fourcc=fourcc, class_mask=class_mask, win_size=win_size,
                         overlap=overlap, tracker=tracker, action_id=action_id, half=half, batch_frames=batch_frames,
                         device_overlay=device_overlay)
