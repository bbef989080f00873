"""Device binding on the GPU box: one process drives one GPU."""
import json
import os
import subprocess
import sys
import threading

import pytest

from yolo_deepsort_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_bound_device_survives_constructors_and_threads():
    from yolo_deepsort_amd import cfgs, synth
    from yolo_deepsort_amd.models import Darknet
    from yolo_deepsort_amd.deep_sort import DeepSort
    dev = _lib.init()
    lib = _lib.load()
    assert lib.yds_current_device() == dev == _lib.current_device()
    net = Darknet(None, img_size=(96, 96), cfg_text=cfgs.cfg_text("yolov3-tiny", 96, 96))
    ds = DeepSort(synth.reid_state_dict(0), use_cuda=True)
    clone = ds.clone()
    assert lib.yds_current_device() == dev and net.device == f"cuda:{dev}"
    assert clone.extractor is ds.extractor and clone.tracker is not ds.tracker       # deep_sort.py:41-44
    assert len(_lib.pci_bus_id()) >= 7
    with pytest.raises(_lib.YdsError):
        _lib.init(dev + 1)
    seen = {}

    def worker():            # hipSetDevice is per host thread: ABI entries re-select the bound device
        buf = _lib.DeviceBuffer(1024)
        seen["dev"] = lib.yds_current_device()
        buf.free()
    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert seen["dev"] == dev


def test_rank_beyond_device_count_fails_loudly():
    """A rank whose LOCAL_RANK has no GPU must raise - never fall back to GPU 0."""
    n = _lib.load().yds_device_count()
    code = ("import sys; sys.path.insert(0, %r)\nfrom yolo_deepsort_amd import _lib\n"
            "try:\n    _lib.init()\nexcept _lib.YdsError as e:\n    print('ERR', e)\nelse:\n    print('BOUND', _lib.current_device())\n" % ROOT)
    env = {k: v for k, v in os.environ.items() if k not in _lib.VISIBILITY_MASKS and k != "YDS_DEVICE"}
    if len(env) != len(os.environ) and n == 1:
        # the box itself masks its devices down to one: then LOCAL_RANK is not an ordinal (see the next-but-one test) and
        # clearing the mask may expose more devices than the count above - ask for a device far outside either way
        n = 64
    out = subprocess.run([sys.executable, "-c", code], env=dict(env, LOCAL_RANK=str(n)), capture_output=True, text=True, timeout=300)
    assert "ERR" in out.stdout and "outside" in out.stdout, out.stdout + out.stderr


def test_two_ranks_use_two_gpus():
    """bench.py --gpus 2 launches itself under torch.distributed.run; each rank must sit on its own GPU."""
    if _lib.load().yds_device_count() < 2:
        pytest.skip("needs 2 GPUs (the driver's 8-GPU node runs the scaling bench)")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--cpu-frames", "0",
                          "--no-roofline"], capture_output=True, text=True, timeout=1200)
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and len(set(line["config"]["rank_pci_bus_ids"])) == 2, line
    assert line["config"]["transport"] == "rccl" and line["config"]["rccl_world"] == 2 and line["config"]["rccl_version"] > 0, line["config"]


def _bench(tmp, extra, env=None, launcher=None):
    cmd = (launcher or [sys.executable]) + [os.path.join(ROOT, "bench.py")] + extra + ["--full", "--cpu-frames", "0", "--no-extras", "--no-roofline", "--latency-steps", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=env or os.environ)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-500:] + out.stderr[-1500:]          # rank 0 prints ONE line
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A run without --full measures the headline only; --dump-outputs holds the rows its LAST timed step returned (the same rows
    --dump-rows records for that step)."""
    import numpy as np
    outs, rows = tmp_path / "outs", str(tmp_path / "rows.npz")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "cfg2", "--steps", "3", "--warmup", "1", "--batch", "4",
           "--dump-rows", rows, "--dump-outputs", str(outs)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-500:] + out.stderr[-1500:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["higher_is_better"] is True
    assert line["unit"] == "frames/s" and line["dtype"] == "f16x3" and line["config"]["frames_per_step"] == 4
    assert abs(line["ms_per_step"] - 4e3 / line["value"]) < 1e-2 * line["ms_per_step"]
    assert not {"roofline", "cpu_baseline", "value_with_upload", "value_frame_by_frame", "value_video_detector"} & set(line)
    r, c = np.load(outs / "track_rows.npy"), np.load(outs / "track_counts.npy")
    assert r.dtype == c.dtype == np.float64 and r.shape[1] == 8 and c.shape == (1, 4) and r.shape[0] > 0
    g = np.load(rows)
    for f in range(4):
        want = g[f"s0_k2_f{f}"]
        if c[0, f] < 0:
            assert np.array_equal(want, np.full((1, 6), -1, np.int32))
        else:
            got = r[r[:, 1] == f]
            assert len(got) == c[0, f] and (got[:, 0] == 0).all() and np.array_equal(got[:, 2:].astype(np.int32), want), f


def test_two_rank_bench_path_on_one_gpu(tmp_path):
    """The N > 1 code path end to end on the 1-GPU box with BASELINE configs[3] (cfg4 = yolov4 + DeepSORT, one stream per rank,
    seeds = rank): two processes under torch.distributed.run, barriers + max-over-ranks timing + the exchange step (all-gather
    of every stream's result rows) - with both ranks bound to GPU 0 and gloo as transport (RCCL refuses two ranks on one
    device; the real run uses RCCL and one GPU per rank).  The rows rank 0 gathered must equal two single-rank runs of
    seeds 0 and 1 bit for bit."""
    import numpy as np
    env = dict(os.environ, YDS_DEVICE="0", YDS_DIST_BACKEND="gloo")
    launcher = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29577"]
    both = str(tmp_path / "both.npz")
    line = _bench(tmp_path, ["--gpus", "2", "--config", "cfg4", "--steps", "2", "--warmup", "1", "--batch", "4", "--dump-rows", both], env, launcher)
    assert line["n_gpus"] == 2 and line["config"]["streams"] == 2 and line["scaling"] == "weak"
    assert line["config"]["rank_devices"] == [0, 0] and line["value"] > 0
    assert "one per GPU" in line["config"]["workload"] and "gloo" in line["exchange"]
    # the run certifies its own transport: machine-readable, not inside a free-text string
    c = line["config"]
    assert c["transport"] == "gloo" and c["requested"] == "gloo" and c["rccl_world"] == 0 and c["rccl_version"] is None
    assert len(c["rank_values"]) == 2 and all(v > 0 for v in c["rank_values"]) and c["exchange_block_rows"] >= 64
    # the N > 1 line explains itself (VERDICT r5 'next' #8): every rank's own ms per step, rank 0 alone before the communicator formed
    # (on a workload of its own: the streams' rows below still equal fresh single-rank runs), and the ratio the two give
    assert len(c["rank_ms_per_step"]) == 2 and all(v > 0 for v in c["rank_ms_per_step"])
    assert c["rank0_single"]["value"] > 0 and c["rank0_single"]["steps"] >= 2
    assert abs(c["efficiency_vs_rank0_single"] - line["value"] / (2 * c["rank0_single"]["value"])) < 1e-3
    g = np.load(both)
    total = 0
    for seed in (0, 1):
        one = str(tmp_path / f"one{seed}.npz")
        _bench(tmp_path, ["--gpus", "1", "--config", "cfg4", "--steps", "2", "--warmup", "1", "--batch", "4", "--seed-base", str(seed), "--dump-rows", one])
        h = np.load(one)
        keys = sorted(k for k in g.files if k.startswith(f"s{seed}_"))
        assert keys and sorted(h.files) == sorted(k.replace(f"s{seed}_", "s0_") for k in keys)
        for k in keys:
            assert np.array_equal(g[k], h[k.replace(f"s{seed}_", "s0_")]), (seed, k)
            total += int((g[k][:, 4] >= 0).sum())
    assert total == line["config"]["tracker_rows_out"] and total > 0                            # rank 0 holds BOTH streams' rows


def test_eight_rank_bench_path_on_one_gpu(tmp_path):
    """De-risks the driver's 8-GPU line on the 1-GPU box (VERDICT r4 'next' #7): `bench.py --gpus 8 --config cfg4` as EIGHT processes under
    torch.distributed.run - the 8-way rendezvous, eight concurrent plan-time autotunes (sharing one YDS_TUNE_CACHE file: concurrent
    appends and reads), eight schedule trials, the exchange step over eight blocks per frame with an exchange block that starts
    too small (YDS_EXCHANGE_ROWS=8: it has to grow in the first steps) - all ranks bound to GPU 0, gloo as transport (RCCL refuses
    ranks sharing a device; the real run has one GPU per rank and RCCL).  Every stream's rows, as gathered on rank 0, must equal a
    single-rank run of that seed bit for bit (reference: one DeepSort.clone() per stream, deep_sort/deep_sort.py:41-44)."""
    import numpy as np
    N = 8
    cache = str(tmp_path / "tune.txt")
    env = dict(os.environ, YDS_DEVICE="0", YDS_DIST_BACKEND="gloo", YDS_TUNE_CACHE=cache, YDS_EXCHANGE_ROWS="8")
    launcher = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={N}", "--master-addr", "127.0.0.1", "--master-port", "29591"]
    allp = str(tmp_path / "all.npz")
    args = ["--config", "cfg4", "--steps", "3", "--warmup", "1", "--batch", "4"]
    line = _bench(tmp_path, ["--gpus", str(N)] + args + ["--dump-rows", allp], env, launcher)
    c = line["config"]
    assert line["n_gpus"] == N and c["streams"] == N and line["scaling"] == "weak" and line["value"] > 0
    assert c["rank_devices"] == [0] * N and c["transport"] == "gloo" and len(c["rank_values"]) == N and all(v > 0 for v in c["rank_values"])
    assert c["exchange_block_rows"] == 64, c["exchange_block_rows"]          # grew from 8 rows (a frame here has ~30) to the next multiple of 64
    assert os.path.getsize(cache) > 0
    g = np.load(allp)
    total = 0
    env1 = dict(os.environ, YDS_TUNE_CACHE=cache)                             # (the single-rank runs read the choices the eight wrote)
    for seed in range(N):
        one = str(tmp_path / f"one{seed}.npz")
        _bench(tmp_path, ["--gpus", "1"] + args + ["--seed-base", str(seed), "--dump-rows", one], env1)
        h = np.load(one)
        keys = sorted(k for k in g.files if k.startswith(f"s{seed}_"))
        assert keys and sorted(h.files) == sorted(k.replace(f"s{seed}_", "s0_") for k in keys), seed
        for k in keys:
            assert np.array_equal(g[k], h[k.replace(f"s{seed}_", "s0_")]), (seed, k)
            total += int((g[k][:, 4] >= 0).sum())
    assert total == c["tracker_rows_out"] and total > 0


def test_rccl_failure_fails_the_multi_gpu_bench(tmp_path):
    """Two ranks on ONE device with the RCCL backend asked for (the default): both ranks pass the local preflight, rank 0 creates the
    id, both call ncclCommInitRank, RCCL refuses (duplicate GPU).  Every rank agrees on the outcome over the host group (no rank is
    left inside the collective) - and bench.py must then REFUSE to measure: a scaling run must not go green on gloo by accident."""
    env = dict(os.environ, YDS_DEVICE="0")
    env.pop("YDS_DIST_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29583",
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "cfg4", "--steps", "2", "--warmup", "1", "--batch", "4",
           "--full", "--cpu-frames", "0", "--no-extras", "--no-roofline", "--latency-steps", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode != 0, out.stdout[-500:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and "error" in lines[0] and "RCCL" in lines[0]["error"] and "value" not in lines[0], lines


def test_rccl_refusal_leaves_every_rank_on_the_host_group(tmp_path):
    """The library level of the same situation: Ranks.connect() on two ranks sharing one device ends with BOTH ranks on gloo (same
    decision everywhere, reason recorded), and the exchange step still works there."""
    code = r'''
import os, sys
sys.path.insert(0, %r)
import numpy as np
from yolo_deepsort_amd import _lib
from yolo_deepsort_amd.dist import Ranks
r = Ranks("nccl")
_lib.init()
r.connect()
d = r.describe()
assert d["transport"] == "gloo" and d["requested"] == "nccl" and d["rccl_world"] == 0 and d["fallback_reason"], d
rows = r.gather_rows([np.full((r.rank + 1, 6), r.rank, np.int32)])
assert rows[0][0].shape == (1, 6) and rows[1][0].shape == (2, 6)
if r.rank == 0:
    print("OK", d["fallback_reason"][:80])
r.shutdown()
''' % ROOT
    script = tmp_path / "fallback.py"
    script.write_text(code)
    env = dict(os.environ, YDS_DEVICE="0")
    env.pop("YDS_DIST_BACKEND", None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29585", str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-800:] + out.stderr[-2000:]


def test_rccl_comm_world_of_one():
    """yds_comm_* on RCCL itself (ncclCommInitRank / ncclAllGather / ncclAllReduce) - a world of one rank is all a 1-GPU box
    can form; the collectives must round-trip the exchange block and the reductions."""
    import ctypes as C
    import numpy as np
    from yolo_deepsort_amd import dist
    _lib.init()
    lib = _lib.load()
    assert lib.yds_comm_rccl_version() > 0
    ident = (C.c_char * 128)()
    _lib.check(lib.yds_comm_unique_id(ident))
    comm = _lib.check_ptr(lib.yds_comm_create(ident, 1, 0))
    try:
        assert lib.yds_comm_world(comm) == 1 and lib.yds_comm_rank(comm) == 0
        outs = [np.arange(12, dtype=np.int32).reshape(2, 6), None, np.zeros((0, 6), np.int32), np.full((256, 6), 7, np.int32)]
        blk = dist.pack_rows(outs, dist.rows_for(256))
        back = np.zeros((1,) + blk.shape, np.int32)
        _lib.check(lib.yds_comm_allgather(comm, _lib.ptr(blk), blk.nbytes, _lib.ptr(back)))
        got = dist.unpack_rows(back[0])
        assert got[1] is None and all(np.array_equal(a, b) for a, b in zip([got[0], got[2], got[3]], [outs[0], outs[2], outs[3]]))
        # the C-side packer from the pipeline's own output layout (out6 [batch, cap, 6] + counts)
        cap = 300
        out6 = np.zeros((3, cap, 6), np.int32)
        out6[0, :2] = outs[0]
        counts = np.array([2, -1, 0], np.int32)
        allb = np.zeros((1, 3, dist.block_ints(64)), np.int32)
        need = C.c_int(-1)
        _lib.check(lib.yds_comm_allgather_rows(comm, _lib.ptr(out6), cap, _lib.ptr(counts), 3, 64, _lib.ptr(allb), C.byref(need)))
        assert need.value == 2
        rows = dist.unpack_rows(allb[0])
        assert np.array_equal(rows[0], outs[0]) and rows[1] is None and rows[2].shape == (0, 6)
        v = (C.c_double * 2)(3.5, -1.0)
        _lib.check(lib.yds_comm_allreduce_f64(comm, v, 2, 1))
        assert list(v) == [3.5, -1.0]
        _lib.check(lib.yds_comm_allreduce_f64(comm, v, 2, 0))
        assert list(v) == [3.5, -1.0]
        _lib.check(lib.yds_comm_barrier(comm))
        # device-side variant
        buf = _lib.DeviceBuffer.from_array(blk)
        dst = _lib.DeviceBuffer(blk.nbytes)
        _lib.check(lib.yds_comm_allgather_dev(comm, buf.ptr, blk.nbytes, dst.ptr))
        back2 = np.zeros_like(blk)
        _lib.check(lib.yds_memcpy_d2h(_lib.ptr(back2), dst.ptr, blk.nbytes))
        assert np.array_equal(back2, blk)
        # a frame that does not fit announces its size instead of failing; the caller repeats with a grown block
        many = np.arange(cap * 6, dtype=np.int32).reshape(1, cap, 6)
        small = np.zeros((1, 1, dist.block_ints(64)), np.int32)
        _lib.check(lib.yds_comm_allgather_rows(comm, _lib.ptr(many), cap, _lib.ptr(np.array([257], np.int32)), 1, 64, _lib.ptr(small), C.byref(need)))
        assert need.value == 257 and small[0, 0, 0] == -259
        R = dist.rows_for(need.value)
        grown = np.zeros((1, 1, dist.block_ints(R)), np.int32)
        _lib.check(lib.yds_comm_allgather_rows(comm, _lib.ptr(many), cap, _lib.ptr(np.array([257], np.int32)), 1, R, _lib.ptr(grown), C.byref(need)))
        assert np.array_equal(dist.unpack_rows(grown[0])[0], many[0, :257])
        assert lib.yds_comm_allgather_rows(comm, _lib.ptr(many), cap, _lib.ptr(np.array([cap + 1], np.int32)), 1, R, _lib.ptr(grown), C.byref(need)) != 0
        assert "holds" in _lib.last_error()
        assert lib.yds_comm_preflight() == 0
        assert lib.yds_comm_barrier(None) != 0 and "null" in _lib.last_error()
    finally:
        lib.yds_comm_destroy(comm)


def test_masked_rank_takes_its_only_visible_device():
    """A launcher that masks the devices per rank (HIP_VISIBLE_DEVICES = one GPU each) leaves LOCAL_RANK = 3 with ordinal 0."""
    code = ("import sys; sys.path.insert(0, %r)\nfrom yolo_deepsort_amd import _lib\nprint('BOUND', _lib.init(), _lib.pci_bus_id())\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LOCAL_RANK="3", HIP_VISIBLE_DEVICES="0"), capture_output=True, text=True, timeout=300)
    assert "BOUND 0" in out.stdout, out.stdout + out.stderr


SINGLE_STREAM = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from yolo_deepsort_amd import _lib, cfgs, synth
from yolo_deepsort_amd.dist import Ranks
from yolo_deepsort_amd.models import Darknet
from yolo_deepsort_amd.detect import ImageDetector
from yolo_deepsort_amd.deep_sort import DeepSort
from yolo_deepsort_amd.single_stream import SingleStream
ranks = Ranks(os.environ.get("YDS_DIST_BACKEND", "nccl"))
_lib.init()
ranks.connect()
cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
net = Darknet(None, img_size=(416, 416), cfg_text=cfg)
net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0, 1.0))
names = %(names)r
det = ImageDetector(net, names, thres=0.5, nms_thres=0.4)
ds = DeepSort(synth.reid_state_dict(0), use_cuda=True, max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)
scene = synth.PersonScene(6, frame_hw=(270, 480), seed=3, occlude_frac=0.0)
frames = [scene.frame(t) for t in range(9)]
out = SingleStream.from_components(ranks, det, ds, class_mask=[0, 2, 4]).run(frames)
if ranks.rank == 0:
    arrays = {f"f{t}": (np.full((1, 6), -1, np.int32) if o is None else np.asarray(o, np.int32).reshape(-1, 6)) for t, o in enumerate(out)}
    np.savez(%(dump)r, **arrays)
    print("OK", len(out))
ranks.shutdown()
'''


def test_single_stream_mode_two_ranks_equals_one_process(tmp_path):
    """SURVEY 8e optional mode: ONE stream, frames detected + embedded round-robin on two ranks (both on GPU 0 here, gloo
    transport), fixed-size (tlwh, payload, feats) blocks all-gathered, tracker on rank 0 in frame order - the rows must equal
    the same script run as a single rank (which is the plain frame-by-frame loop)."""
    import numpy as np
    from yolo_deepsort_amd import cfgs
    names = str(tmp_path / "coco.names")
    open(names, "w").write(cfgs.coco_names_text())
    res = {}
    for world in (2, 1):
        dump = str(tmp_path / f"rows{world}.npz")
        script = tmp_path / f"run{world}.py"
        script.write_text(SINGLE_STREAM % dict(root=ROOT, names=names, dump=dump))
        env = dict(os.environ, YDS_DEVICE="0", YDS_DIST_BACKEND="gloo")
        if world == 2:
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29581", str(script)]
        else:
            cmd = [sys.executable, str(script)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
        assert out.returncode == 0 and "OK 9" in out.stdout, out.stdout[-800:] + out.stderr[-2000:]
        res[world] = np.load(dump)
    rows = 0
    for t in range(9):
        assert np.array_equal(res[2][f"f{t}"], res[1][f"f{t}"]), t
        rows += int((res[1][f"f{t}"][:, 4] >= 0).sum())
    assert rows > 0


def test_single_stream_device_exchange_world_of_one():
    """Round 4: the single-stream mode with the embeddings kept in HBM - feature rows staged per frame in a device block, all-gathered
    device to device over RCCL (a world of one is all this box can form) and read by the tracker from the gathered buffer - gives
    the rows of the host-block form, for rounds of 1 and of 3 frames per rank."""
    import ctypes as C
    import numpy as np
    from yolo_deepsort_amd import cfgs, synth
    from yolo_deepsort_amd.dist import Ranks
    from yolo_deepsort_amd.models import Darknet
    from yolo_deepsort_amd.detect import ImageDetector
    from yolo_deepsort_amd.deep_sort import DeepSort
    from yolo_deepsort_amd.single_stream import SingleStream
    import tempfile
    _lib.init()
    lib = _lib.load()
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0, 1.0))
    with tempfile.NamedTemporaryFile("w", suffix=".names", delete=False) as f:
        f.write(cfgs.coco_names_text())
        names = f.name
    det = ImageDetector(net, names, thres=0.5, nms_thres=0.4)
    scene = synth.PersonScene(6, frame_hw=(270, 480), seed=3, occlude_frac=0.0)
    frames = [scene.frame(t) for t in range(8)]

    def tracker():
        return DeepSort(synth.reid_state_dict(0), use_cuda=True, max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)

    def rows(o):
        return [None if x is None else np.asarray(x, np.int32).reshape(-1, 6) for x in o]

    ranks = Ranks("gloo")                                         # no launcher: one rank
    want = rows(SingleStream.from_components(ranks, det, tracker(), class_mask=[0, 2, 4], device=False).run(frames))
    assert sum(len(x) for x in want if x is not None) > 0
    ident = (C.c_char * 128)()
    _lib.check(lib.yds_comm_unique_id(ident))
    ranks.comm = _lib.check_ptr(lib.yds_comm_create(ident, 1, 0))
    try:
        for B in (1, 3):
            S = SingleStream.from_components(ranks, det, tracker(), class_mask=[0, 2, 4], frames_per_rank=B, device=True)
            assert S.on_device
            got = rows(S.run(frames))
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert (a is None and b is None) or np.array_equal(a, b)
            assert (len(frames) + B - 1) // B <= S.exchanges <= (len(frames) + B - 1) // B + 2     # one per round (+ a repeat when the block grows)
    finally:
        lib.yds_comm_destroy(ranks.comm)
        ranks.comm = None
        os.unlink(names)
