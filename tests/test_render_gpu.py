"""Display images on the device (include/dspn_render.h) against tests/ref_render.py: every comparison is exact, on uint8.
Canvases start from a pattern, so a byte written outside the panel shows.  Shapes are the smallest at which each thing can
go wrong: odd byte strides and unaligned panel starts (37 x 53 canvas, panel at (3, 5)), the aligned x4 case, one row wide
enough for several workgroups in x, both channel-read paths of the class map, and a draw table longer than one LDS chunk."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_render as ref  # noqa: E402

from dspnet_amd import functional as fn  # noqa: E402
from dspnet_amd.detect import render as R  # noqa: E402

pytestmark = pytest.mark.gpu

CLASSES = ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
# (h, w, Hd, Wd, CH, CW, y0, x0)
GEOMETRIES = [(5, 7, 13, 17, 37, 53, 3, 5),            # odd strides, unaligned start, a general scale
              (8, 16, 32, 64, 32, 64, 0, 0),           # exactly x4, the panel is the canvas, every row aligned
              (1, 300, 1, 1200, 3, 1203, 1, 2)]        # one row across several workgroups


def pattern(B, CH, CW):
    return ((np.arange(B * CH * CW * 3, dtype=np.int64) * 7 + 3) % 251).astype(np.uint8).reshape(B, CH, CW, 3)


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def consts(device):
    return dev(R.palette_table().reshape(-1), device), dev(np.frombuffer(R.FONT, np.uint8).copy(), device)


def tables(h, w, Hd, Wd, device):
    ys, xs = R.nearest_tables(h, w, Hd, Wd)
    return ys, xs, dev(ys, device), dev(xs, device)


@pytest.mark.parametrize("ld", [20, 23])               # 16-byte channel loads / scalar loads
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_classmap(gpu_device, geom, ld):
    h, w, Hd, Wd, CH, CW, y0, x0 = geom
    B, C = 2, 19
    g = np.random.Generator(np.random.PCG64(11))
    scores = g.random((B, h, w, ld), dtype=np.float32)
    scores[..., C:] = 1e30                              # the pad lanes would win every comparison they entered
    flat = scores.reshape(-1, ld)
    for i in range(0, flat.shape[0], 3):                # ties between two classes: the first wins
        a, b = sorted(g.choice(C, 2, replace=False))
        flat[i, a] = flat[i, b] = 2.0
    flat[1, :C] = 0.5                                   # all equal: class 0
    flat[2, C - 1] = 3.0                                # the last channel that counts
    want = pattern(B, CH, CW)
    ys, xs, ysd, xsd = tables(h, w, Hd, Wd, gpu_device)
    ref.classmap(scores, C, R.palette_table(), ys, xs, want, y0, x0)
    canvas = dev(pattern(B, CH, CW), gpu_device)
    pal, _ = consts(gpu_device)
    fn.render_classmap(dev(scores, gpu_device), C, pal, ysd, xsd, canvas, y0, x0)
    np.testing.assert_array_equal(canvas.cpu().numpy(), want)
    assert (want[:, y0:y0 + Hd, x0:x0 + Wd] != pattern(B, CH, CW)[:, y0:y0 + Hd, x0:x0 + Wd]).any()


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_labels(gpu_device, geom):
    h, w, Hd, Wd, CH, CW, y0, x0 = geom
    B = 2
    g = np.random.Generator(np.random.PCG64(12))
    values = np.array(list(range(19)) + [255], np.float32)
    label = values[g.integers(0, 20, size=(B, h, w))]
    n = min(20, label.size)
    label.reshape(-1)[:n] = values[:n]                  # every value at least once
    want = pattern(B, CH, CW)
    ys, xs, ysd, xsd = tables(h, w, Hd, Wd, gpu_device)
    ref.labels(label, R.palette_table(), ys, xs, want, y0, x0)
    canvas = dev(pattern(B, CH, CW), gpu_device)
    pal, _ = consts(gpu_device)
    fn.render_labels(dev(label, gpu_device), pal, ysd, xsd, canvas, y0, x0)
    np.testing.assert_array_equal(canvas.cpu().numpy(), want)


@pytest.mark.parametrize("cmap", [(2, 1, 0), (0, 1, 2)])
def test_data_panel(gpu_device, cmap):
    B, H, W, CH, CW, y0, x0 = 2, 13, 21, 37, 53, 3, 5
    sub = np.array([123, 117, 104], np.float32)
    planes = np.zeros((B, 3, H * W), np.float32)
    v = np.arange(256, dtype=np.float32)
    for p in range(3):
        planes[:, p, :256] = v - sub[p]                 # every grey level, as the iterator leaves it
    extra = np.array([-1000.0, -124.0, -123.7, -0.5, 151.5, 152.0, 300.0, 1e9, -1e9, 0.25, 131.321, 138.221, 151.061, 3e38, -3e38, 1.0, 2.0],
                     np.float32)
    planes[0, :, 256:] = extra                          # beyond 0..255: saturation; and values just under a grey level
    planes[1, :, 256:] = extra[::-1]
    planes = planes.reshape(B, 3, H, W)
    want = pattern(B, CH, CW)
    ref.data(planes, cmap, R.DISPLAY_MEAN, want, y0, x0)
    if cmap == (0, 1, 2):
        # 123.68 / 116.779 / 103.939 added to data that had 123 / 117 / 104 subtracted: green comes back one level low
        flat = want[0, y0:y0 + H, x0:x0 + W].reshape(-1, 3)[:256]
        np.testing.assert_array_equal(flat[:, 0], np.arange(256))
        np.testing.assert_array_equal(flat[:, 1], np.maximum(np.arange(256) - 1, 0))
        np.testing.assert_array_equal(flat[:, 2], np.maximum(np.arange(256) - 1, 0))
    canvas = dev(pattern(B, CH, CW), gpu_device)
    fn.render_data(dev(planes, gpu_device), cmap, R.DISPLAY_MEAN, canvas, y0, x0)
    np.testing.assert_array_equal(canvas.cpu().numpy(), want)


def O(x0, y0, x1, y1, rgb, t=1):
    return (fn.DRAW_OUTLINE, x0, y0, x1, y1) + tuple(rgb) + (t,)


def F(x0, y0, x1, y1, rgb):
    return (fn.DRAW_FILL, x0, y0, x1, y1) + tuple(rgb) + (0,)


def G(x, y, code, s, rgb):
    return (fn.DRAW_GLYPH, x, y, 0, 0) + tuple(rgb) + ((s << 8) | code,)


def small_draw_list():
    image0 = [F(2, 2, 20, 12, (200, 10, 10)), O(5, 5, 30, 20, (10, 200, 10), 1), F(10, 8, 14, 30, (10, 10, 200)),
              O(8, 3, 25, 15, (250, 250, 0), 2), O(28, 18, 12, 6, (0, 250, 250), 3),        # swapped corners
              O(-4, -3, 6, 5, (90, 90, 90), 3), F(45, 30, 70, 50, (1, 2, 3)),                # partly outside
              F(60, 10, 80, 20, (9, 9, 9)), O(-30, -30, -10, -10, (9, 9, 9), 2), F(5, 40, 9, 60, (9, 9, 9)),   # wholly outside
              F(33, 3, 33, 3, (255, 255, 255)), O(35, 3, 35, 3, (255, 0, 255), 1),           # one pixel
              O(40, 2, 41, 3, (5, 5, 5), 1), O(44, 2, 46, 4, (7, 7, 7), 3),                  # nothing left inside
              G(3, 22, ord("R"), 1, (255, 255, 255)), G(10, 21, ord("g"), 2, (255, 128, 0)),
              G(48, 5, ord("W"), 2, (0, 255, 0)), G(30, 31, ord("8"), 1, (0, 0, 255)),       # clipped at the right / bottom edge
              G(44, 28, ord("#"), 2, (200, 200, 200)), G(-3, -2, ord("M"), 1, (1, 1, 1)),
              G(20, 24, 7, 1, (128, 128, 128)), G(27, 24, 200, 1, (64, 64, 64)),             # codes outside 32..126: the block
              F(11, 22, 13, 25, (33, 44, 55))]                                               # over the glyph drawn before it
    image2 = [F(2, 2, 20, 12, (3, 30, 130)), O(5, 5, 30, 20, (130, 30, 3), 2), G(3, 22, ord("Q"), 1, (9, 99, 199))]
    return [image0, [], image2]


@pytest.mark.parametrize("panel", [None, (3, 5, 29, 41)])
def test_draw_list_painters_order(gpu_device, panel):
    B, CH, CW = 3, 37, 53
    rows = small_draw_list()
    y0, x0, Hd, Wd = panel or (0, 0, CH, CW)
    font = np.frombuffer(R.FONT, np.uint8)
    want = pattern(B, CH, CW)
    ref.draw_list(want, rows, font, y0, x0, Hd, Wd)
    back = pattern(B, CH, CW)
    ref.draw_list(back, [r[::-1] for r in rows], font, y0, x0, Hd, Wd)
    assert (back[0] != want[0]).any()                   # the reverse order is another picture
    np.testing.assert_array_equal(want[1], pattern(B, CH, CW)[1])       # image 1 owns no rows
    assert (want[2] != want[0]).any()
    canvas = dev(pattern(B, CH, CW), gpu_device)
    _, fontd = consts(gpu_device)
    fn.render_draw_list(canvas, fn.draw_table(rows, gpu_device), fontd, y0, x0, Hd, Wd)
    np.testing.assert_array_equal(canvas.cpu().numpy(), want)


def test_draw_list_longer_than_one_chunk(gpu_device):
    chunk = fn.render_chunk_rows()
    B, CH, CW = 2, 37, 53
    g = np.random.Generator(np.random.PCG64(13))
    rows = []
    for i in range(2 * chunk + 17):
        x, y = int(g.integers(-5, CW)), int(g.integers(-5, CH))
        rgb = tuple(int(v) for v in g.integers(0, 256, 3))
        kind = i % 3
        if kind == 0:
            rows.append(O(x, y, x + int(g.integers(0, 25)), y + int(g.integers(0, 25)), rgb, 1 + i % 4))
        elif kind == 1:
            rows.append(F(x, y, x + int(g.integers(0, 12)), y + int(g.integers(0, 12)), rgb))
        else:
            rows.append(G(x, y, int(g.integers(30, 130)), 1 + i % 2, rgb))
    for k in (chunk, 2 * chunk):                        # the same area on both sides of a chunk boundary
        rows[k - 1] = F(20, 10, 40, 30, (1, 1, k % 256))
        rows[k] = F(25, 5, 35, 35, (2, 2, k % 256))
    per_image = [rows[:5], rows]                        # image 1 starts inside the table, not on a chunk boundary
    font = np.frombuffer(R.FONT, np.uint8)
    want = pattern(B, CH, CW)
    ref.draw_list(want, per_image, font)
    canvas = dev(pattern(B, CH, CW), gpu_device)
    _, fontd = consts(gpu_device)
    fn.render_draw_list(canvas, fn.draw_table(per_image, gpu_device), fontd)
    np.testing.assert_array_equal(canvas.cpu().numpy(), want)


def test_same_bytes_on_a_second_run_and_on_another_stream(gpu_device):
    B, CH, CW = 3, 37, 53
    pal, fontd = consts(gpu_device)
    g = np.random.Generator(np.random.PCG64(14))
    scores = dev(g.random((B, 5, 7, 20), dtype=np.float32), gpu_device)
    planes = dev((g.random((B, 3, 13, 17), dtype=np.float32) * 300 - 150).astype(np.float32), gpu_device)
    _, _, ysd, xsd = tables(5, 7, 13, 17, gpu_device)
    table = fn.draw_table(small_draw_list(), gpu_device)

    def run():
        canvas = dev(pattern(B, CH, CW), gpu_device)
        fn.render_data(planes, (2, 1, 0), R.DISPLAY_MEAN, canvas, 20, 30)
        fn.render_classmap(scores, 19, pal, ysd, xsd, canvas, 3, 5)
        fn.render_draw_list(canvas, table, fontd)
        fn.render_draw_list(canvas, table, fontd)       # twice on one stream: the picture does not change
        return canvas

    first = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    assert torch.equal(first, second)


# ---------------------------------------------------------------------------------------------- end to end
S = 128


@pytest.fixture(scope="module")
def detector(gpu_device):
    from dspnet_amd import synthetic
    from dspnet_amd.detect.multitask_detector import Detector
    det = Detector("resnet-50", S, num_classes=8, batch_size=2, device=gpu_device, seed=3)
    data = torch.from_numpy(synthetic.images(2, S, S, synthetic.rng(5))).to(gpu_device)
    det_out, seg_prob = det.forward(data)
    return det, data, det_out.clone(), seg_prob.clone()


def planted_detections():
    """rows that are certainly drawn, whatever the synthetic weights detect"""
    d = -np.ones((2, 6, 7), np.float32)
    d[0, 0] = [2, 0.9, 0.1, 0.2, 0.6, 0.7, 0.1]
    d[0, 1] = [0, 0.8, 0.3, 0.3, 0.9, 0.95, 0.4]
    d[0, 2] = [5, 0.3, 0.0, 0.0, 0.5, 0.5, 0.2]         # under the threshold
    d[0, 4] = [7, 0.99, 0.5, 0.1, 1.1, 0.4, 0.3]        # leaves the frame on the right
    d[1, 0] = [1, 0.7, 0.05, 0.5, 0.3, 0.9, 0.05]
    return d


def test_visualize_detection_is_the_composition_of_the_reference_functions(detector):
    det, data, det_out, seg_prob = detector
    seg_np, data_np = seg_prob.cpu().numpy(), data.cpu().numpy()
    for dets, thresh in ((det_out.cpu().numpy(), 0.02), (planted_detections(), 0.6)):
        got = det.visualize_detection(data, torch.from_numpy(dets), seg_prob, CLASSES, thresh)
        assert got.shape == (2, S + S + 30, S, 3) and got.dtype == torch.uint8 and got.is_cuda
        want = ref.visualize_detection(data_np, list(dets), seg_np, CLASSES, thresh, mean=det.mean_pixels)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    # the planted boxes are in the picture: the car's outline colour on its top edge, thickness 1 at 128 rows
    assert tuple(want[0, int(0.2 * S), int(0.1 * S) + 20]) == R.PALETTE[13]
    # uint8 frames take the place of the net's input
    frames = torch.from_numpy(pattern(2, S, S)).to(data.device)
    got = det.visualize_detection(frames, planted_detections(), seg_prob, CLASSES, 0.6)
    want = ref.visualize_detection(pattern(2, S, S), list(planted_detections()), seg_np, CLASSES, 0.6)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_detect_and_visualize_frames(detector):
    det, _, _, _ = detector
    g = np.random.Generator(np.random.PCG64(15))
    frames = g.integers(0, 256, size=(2, 90, 160, 3), dtype=np.uint8)            # 16:9 BGR frames, on the host
    got = det.detect_and_visualize(frames, CLASSES, thresh=0.02)
    assert got.shape == (2, S + S + 30, S, 3) and got.dtype == torch.uint8
    data = det.net.data.data
    shown = np.zeros((2, S, S, 3), np.uint8)
    ref.data(data.cpu().numpy(), (0, 1, 2), det.mean_pixels, shown)
    assert shown.std() > 10                                                       # the warped frame, not a constant
    from dspnet_amd.detect.nms import nms
    det_out = det.net.det.out.data.cpu().numpy()
    rows = []
    for d in det_out:
        d = d[d[:, 0] >= 0]
        rows.append(d[nms(np.hstack((d[:, 2:6], d[:, 1:2])), 0.95)])
    want = ref.visualize_detection(data.cpu().numpy(), rows, det.net.seg_out.prob.data.cpu().numpy(), CLASSES, 0.02,
                                   mean=det.mean_pixels)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_display_results_is_the_composition_of_the_reference_functions(detector):
    from dspnet_amd import synthetic
    det, data, det_out, seg_prob = detector
    gen = synthetic.rng(6)
    label_seg = synthetic.seg_labels(2, S, S, gen=gen)
    gts = synthetic.det_labels(2, gen=gen, height=S, width=S, first_empty=False)
    dets = [planted_detections()[0][:5], det_out[1].cpu().numpy()]
    dets[1] = dets[1][dets[1][:, 0] >= 0][:50]
    got = R.display_results(data, torch.from_numpy(label_seg).to(data.device), seg_prob, dets, gts, CLASSES)
    assert got.shape == (2, 2 * S, 2 * S, 3) and got.dtype == torch.uint8 and got.is_cuda
    want = ref.display_results(data.cpu().numpy(), label_seg, seg_prob.cpu().numpy(), dets, list(gts), CLASSES)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert (want[:, :S, :S] != want[:, S:, :S]).any()                             # ground-truth boxes above, detections below


def test_evaluate_net_writes_the_result_images(gpu_device, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from dspnet_amd import synthetic
    from dspnet_amd.evaluate.multi_eval import evaluate_net, label_ids
    from dspnet_amd.symbol.multitask_symbol_factory import get_multi_symbol_train
    B, full = 2, (64, 96)
    net = get_multi_symbol_train("resnet-50", S, num_classes=8, batch_size=B, device=gpu_device)
    gen = synthetic.rng(233)
    batches = [{"data": torch.from_numpy(synthetic.images(B, S, S, gen)).to(gpu_device),
                "label_det": torch.from_numpy(synthetic.det_labels(B, gen=gen, height=S, width=S)).to(gpu_device),
                "label_seg": torch.from_numpy(synthetic.seg_labels(B, S, S, gen=gen)).to(gpu_device)} for _ in range(2)]
    batches[0]["fnames"] = ["/data/SegmentationClass/aachen_000000_000019_gtFine_labelTrainIds.png",
                            "/data/SegmentationClass/aachen_000001_000019_gtFine_labelTrainIds.png"]
    seg = ["s%d" % i for i in range(19)]
    quiet = tmp_path / "quiet"
    quiet.mkdir()
    cwd = os.getcwd()
    os.chdir(str(quiet))
    try:
        base = evaluate_net(net, batches, CLASSES, seg, full_res=full)               # results_dir=None: nothing is written
    finally:
        os.chdir(cwd)
    assert os.listdir(str(quiet)) == []
    out_dir = tmp_path / "out"
    out = evaluate_net(net, batches, CLASSES, seg, full_res=full, results_dir=str(out_dir))
    assert set(out) == set(base)                        # the same metrics, and their values do not move
    for k in ("CrossEntropy", "SmoothL1", "accuracy", "mAP", "mIoU"):
        assert out[k] == base[k] or (np.isnan(out[k]) and np.isnan(base[k])), k
    names = ["aachen_000000_000019_gtFine_labelTrainIds.png", "aachen_000001_000019_gtFine_labelTrainIds.png",
             "000002_gtFine_labelTrainIds.png", "000003_gtFine_labelTrainIds.png"]
    assert sorted(os.listdir(str(out_dir))) == ["output", "results"]
    assert sorted(os.listdir(str(out_dir / "results"))) == sorted(names)
    assert sorted(os.listdir(str(out_dir / "output"))) == sorted(n.replace("labelTrainIds", "output") for n in names)
    ids = np.asarray(Image.open(str(out_dir / "results" / names[3])))
    np.testing.assert_array_equal(ids, label_ids(out["class_maps"][1][1]).cpu().numpy())
    # the last batch is still in the graph: the mosaic file of its second image is display_results of those tensors
    mosaic = np.asarray(Image.open(str(out_dir / "output" / names[3].replace("labelTrainIds", "output"))))
    from dspnet_amd.evaluate.multi_eval import filter_detections
    want = ref.display_results(net.data.data.cpu().numpy(), net.label_seg.data.cpu().numpy(), net.seg_out.prob.data.cpu().numpy(),
                               list(filter_detections(net.det.out.data, 0.1)), list(net.label_det.data.cpu().numpy()), CLASSES)
    assert mosaic.shape == (2 * S, 2 * S, 3)
    np.testing.assert_array_equal(mosaic, want[1])
