"""MultiBoxTarget / MultiBoxDetection alone at the bench shapes (9 classes, the resnet-50 anchor table of the given input
size), written to profiles/ by hand from this script's output: event-timed totals; run under rocprofv3 --kernel-trace
--stats for the per-kernel split.  Everything is generated from seeds.

    python tools/multibox_measure.py                       # B 32, 512 x 512: 6132 anchors, target_match_reg_kernel<8>
    python tools/multibox_measure.py --size 512 1024       # 12264 anchors: more than 8192, target_match_kernel
    DSPN_LIB=other/libdspn_hip.so python tools/multibox_measure.py     # another build of the library (dspnet_amd/_lib.py)

Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main(args):
    import torch
    from dspnet_amd import _lib, synthetic
    from dspnet_amd import operator as op
    from dspnet_amd.symbol.multitask_symbol_factory import get_config
    dev = torch.device("cuda", 0)
    B, (H, W) = args.batch, args.size
    # the resnet-50 graph's anchor table: the stride-16 and stride-32 maps, then four 3x3 stride-2 pad-1 extras
    cfg = get_config("resnet-50", (3, H, W))
    maps = [(H // 16, W // 16), (H // 32, W // 32)]
    for _ in range(4):
        maps.append(((maps[-1][0] - 1) // 2 + 1, (maps[-1][1] - 1) // 2 + 1))
    anchors = torch.cat([op.MultiBoxPrior(hw, sizes=s, ratios=r).to(dev)
                         for hw, s, r in zip(maps, cfg["sizes"][1:], cfg["ratios"][1:])], dim=1)
    A = anchors.shape[1]
    torch.manual_seed(7)
    lab = torch.from_numpy(synthetic.det_labels(B, gen=synthetic.rng(7))).to(dev)
    pred = torch.randn(B, 9, A, device=dev)
    prob = torch.softmax(pred, dim=1).contiguous()
    loc = 0.1 * torch.randn(B, A * 5, device=dev)
    det_out = torch.empty(B, A, 7, device=dev)
    print("B %d A %d (%d x %d)  %s" % (B, A, H, W, _lib.LIB_PATH))
    rows = [("MultiBoxTarget     %.4f ms", lambda: op.MultiBoxTarget(anchors, lab, pred, negative_mining_ratio=3)),
            ("MultiBoxDetection  %.4f ms (topk 400)", lambda: op.MultiBoxDetection(prob, loc, anchors, nms_topk=400, out=det_out)),
            ("MultiBoxDetection  %.4f ms (threshold 0.2)",
             lambda: op.MultiBoxDetection(prob, loc, anchors, threshold=0.2, nms_topk=400, out=det_out)),
            ("MultiBoxDetection  %.4f ms (force)", lambda: op.MultiBoxDetection(prob, loc, anchors, force_suppress=True, out=det_out))]
    for text, fn in rows:
        print(text % timed(fn, args.reps))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, nargs=2, default=(512, 512), metavar=("H", "W"), help="input height and width")
    ap.add_argument("--reps", type=int, default=20)
    main(ap.parse_args())
