"""worker for tests/test_boxes_gpu.py: lio.Boxes.postprocess_device over torch tensors' data_ptr() against postprocess over the same host
arrays, bit for bit.  A process of its own because torch is imported and initialised BEFORE liblio_hip.so is loaded (the order bench.py uses):
a pytest process has loaded the library long before."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "lidar-slam-detection_amd", "python"), os.path.join(ROOT, "tests")]


def main():
    import torch

    torch.cuda.init()
    import boxes_cases as bc
    from lsd_amd import lio

    G = bc.load_golden()
    b, s, lab, ct = G["post_boxes"], G["post_scores"], G["post_labels"], G["post_class_thresh"]
    bx = lio.Boxes(256)
    host = bx.postprocess(b, s, lab, ct, 0.25, 256)
    tb, ts, tl = torch.from_numpy(b).cuda().contiguous(), torch.from_numpy(s).cuda().contiguous(), torch.from_numpy(lab).cuda().contiguous()
    torch.cuda.synchronize()
    dev = bx.postprocess_device(tb.data_ptr(), ts.data_ptr(), tl.data_ptr(), len(b), ct, 0.25, 256)
    assert len(dev[0]) == len(G["post_keep"]), (len(dev[0]), len(G["post_keep"]))
    for h, d in zip(host, dev):
        assert h.shape == d.shape and np.array_equal(h.view(np.uint32), d.view(np.uint32))
    assert np.array_equal(bx.last_indices(), G["post_keep"])
    bx.close()
    print("boxes torch worker ok")


if __name__ == "__main__":
    main()
