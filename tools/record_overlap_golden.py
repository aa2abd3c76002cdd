#!/usr/bin/env python3
"""Writes tests/golden/overlap.npz: what the reference's matchers (fast_gicp::FastVGICP / FastGICP compiled from the reference tree into
oracle/_ref/libref_gicp.so, configured as select_registration_method("FAST_VGICP") / ("FAST_GICP") with OverlapDetector's max correspondence
distance 0.5 and transformation epsilon 0.001) return for the coarse pairs and the fine alignments of tests/overlap_cases.py's two-map scene,
driven by that file's restatement of OverlapDetector::detect.  Data only.  CPU only.  Run after `make -C oracle ref`:
python tools/record_overlap_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-slam-detection_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import overlap_cases as OC  # noqa: E402
import ref_gicp  # noqa: E402


class RefMatchers:
    def __init__(self):
        self.coarse_log, self.fine_log = [], []

    def coarse(self, target, source, guess):
        m = ref_gicp.RefVgicp(k=20, resolution=1.0, search_method=1, transformation_epsilon=0.1, rotation_epsilon=0.1, max_iterations=64, num_threads=4)
        m.set_target(target)
        m.set_source(source)
        out = m.align(np.asarray(guess, np.float32))
        m.close()
        self.coarse_log.append(out)
        return out

    def fine(self, target, source, guess):
        m = ref_gicp.RefGicp(k=20, max_corr_dist=OC.DEFAULTS["fine_max_corr_dist"], transformation_epsilon=OC.DEFAULTS["fine_translation_epsilon"], max_iterations=64,
                             num_threads=4)
        m.set_target(target)
        m.set_source(source)
        out = m.align(np.asarray(guess, np.float32))
        m.close()
        self.fine_log.append(out)
        return out


def main():
    if not ref_gicp.available():
        raise SystemExit("oracle/_ref/libref_gicp.so is missing: make -C oracle ref")
    M = RefMatchers()
    sc = OC.two_maps()
    edges, recs = OC.detect(sc["clouds"], sc["poses"], sc["ref_ids"], sc["new_ids"], sc["edges"], M)
    pairs, T, it, conv, fine_new, fine_best, fine_nb, fT, fit, fconv, fscore = [], [], [], [], [], [], [], [], [], [], []
    for r in recs:
        for k, c in enumerate(r["candidates"]):
            if r["T"][k] is None:  # the gate refused the pair: the matcher never saw it
                continue
            pairs.append((r["new_id"], c)); T.append(r["T"][k]); it.append(r["iterations"][k]); conv.append(r["converged"][k])
        if r["fine"] is not None:
            fine_new.append(r["new_id"]); fine_best.append(r["candidates"][r["best"]]); fine_nb.append(list(r["neighbours"]) + [-1] * (4 - len(r["neighbours"])))
            fT.append(r["fine"][0]); fit.append(r["fine"][1]); fconv.append(r["fine"][2]); fscore.append(r["fine_score"])
        print(r["new_id"], r["candidates"], r["iterations"], r["converged"], r["best"], r["fine"][1:] if r["fine"] else None, r["fine_score"], r["reason"])
    out = {"coarse/pairs": np.array(pairs, np.int32).reshape(-1, 2), "coarse/T": np.array(T, np.float32).reshape(-1, 4, 4), "coarse/iterations": np.array(it, np.int32),
           "coarse/converged": np.array(conv, bool), "fine/new": np.array(fine_new, np.int32), "fine/best": np.array(fine_best, np.int32),
           "fine/neighbours": np.array(fine_nb, np.int32).reshape(-1, 4), "fine/T": np.array(fT, np.float32).reshape(-1, 4, 4), "fine/iterations": np.array(fit, np.int32),
           "fine/converged": np.array(fconv, bool), "fine/score": np.array(fscore), "edges": np.array([(e["key1"], e["key2"]) for e in edges], np.int32).reshape(-1, 2),
           "n_points": np.array([len(sc["clouds"][k]) for k in sc["ref_ids"] + sc["new_ids"]], np.int64)}
    path = os.path.join(ROOT, "tests", "golden", "overlap.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(pairs), "coarse pairs,", len(fT), "fine alignments, edges", out["edges"].tolist())


if __name__ == "__main__":
    main()
