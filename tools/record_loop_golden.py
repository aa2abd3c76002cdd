#!/usr/bin/env python3
"""Writes tests/golden/loop.npz: what the reference's matchers (fast_gicp::FastVGICP / FastGICP compiled from the reference tree into
oracle/_ref/libref_gicp.so, configured as select_registration_method("FAST_VGICP") / ("FAST_GICP")) and tests/loop_cases.py's restatement of
hdl_graph_slam::LoopDetector give for the two seeded cases of tests/loop_cases.py -- one target with five candidates, and a closed drive of
about 60 key frames.  CPU only.  Run after `make -C oracle ref`:  python tools/record_loop_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lidar-slam-detection_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import loop_cases as LC  # noqa: E402
import ref_gicp  # noqa: E402


class RefMatchers:
    def coarse(self, target, source, guess):
        m = ref_gicp.RefVgicp(k=20, resolution=1.0, search_method=1, transformation_epsilon=0.1, rotation_epsilon=0.1, max_iterations=64, num_threads=4)
        m.set_target(target)
        m.set_source(source)
        out = m.align(np.asarray(guess, np.float32))
        m.close()
        return out

    def fine(self, target, source, guess, max_corr_dist=0.5):
        m = ref_gicp.RefGicp(k=20, max_corr_dist=max_corr_dist, transformation_epsilon=0.01, max_iterations=64, num_threads=4)
        m.set_target(target)
        m.set_source(source)
        out = m.align(np.asarray(guess, np.float32))
        m.close()
        return out


def main():
    if not ref_gicp.available():
        raise SystemExit("oracle/_ref/libref_gicp.so is missing: make -C oracle ref")
    M = RefMatchers()
    out = {}
    # one target, five candidates: the stage door's inputs are the guesses, the selection is matching's
    tgt, cands, guesses = LC.five_candidates()
    T, it, conv, sc, nr = [], [], [], [], []
    for c, g in zip(cands, guesses):
        Tk, itk, ck = M.coarse(tgt, c, g)
        s, n = LC.fitness(tgt, c, Tk) if ck else (LC.DBL_MAX, 0)
        T.append(Tk); it.append(itk); conv.append(ck); sc.append(s); nr.append(n)
    best, best_score = LC.select(conv, sc)
    fT, fit, fconv = M.fine(tgt, cands[best], T[best])
    fs, fnr = LC.fitness(tgt, cands[best], fT)
    out.update({"five/T": np.stack(T).astype(np.float32), "five/iterations": np.array(it, np.int32), "five/converged": np.array(conv, bool),
                "five/score": np.array(sc), "five/nr": np.array(nr, np.int64), "five/best": np.int32(best), "five/fine_T": np.asarray(fT, np.float32),
                "five/fine_iterations": np.int32(fit), "five/fine_converged": np.bool_(fconv), "five/fine_score": np.float64(fs), "five/fine_nr": np.int64(fnr),
                "five/n_points": np.array([len(tgt)] + [len(c) for c in cands], np.int64)})
    print("five:", it, conv, [f"{s:.4g}" for s in sc], "best", best, "fine", fit, fconv, f"{fs:.4g}")
    # the drive: a detect() per key frame, as the wrapper calls it
    det = LC.RefLoopDetector(M)
    for cloud, pose, accum in LC.drive():
        det.add_keyframe(cloud, pose, accum)
        det.detect()
    ms = [m for m in det.matchings if m["candidates"]]
    K = max(len(m["candidates"]) for m in ms)
    pad = lambda a, fill, dt: np.array([list(x) + [fill] * (K - len(x)) for x in a], dt)
    out.update({"drive/new_id": np.array([m["new_id"] for m in ms], np.int32), "drive/n_candidates": np.array([len(m["candidates"]) for m in ms], np.int32),
                "drive/candidates": pad([m["candidates"] for m in ms], -1, np.int32), "drive/iterations": pad([m["iterations"] for m in ms], -1, np.int32),
                "drive/converged": pad([m["converged"] for m in ms], False, bool), "drive/score": pad([m["score"] for m in ms], LC.DBL_MAX, np.float64),
                "drive/best": np.array([m["best"] for m in ms], np.int32), "drive/best_score": np.array([m["best_score"] for m in ms]),
                "drive/fine_ran": np.array([m["fine"] is not None for m in ms], bool),
                "drive/fine_iterations": np.array([m["fine"][1] if m["fine"] else -1 for m in ms], np.int32),
                "drive/fine_converged": np.array([bool(m["fine"][2]) if m["fine"] else False for m in ms], bool),
                "drive/fine_score": np.array([m["fine"][3] if m["fine"] else LC.DBL_MAX for m in ms]),
                "drive/edges": np.array([(e["key1"], e["key2"]) for e in det.edges], np.int32).reshape(-1, 2),
                "drive/edge_pose": np.array([e["relative_pose"] for e in det.edges], np.float32).reshape(-1, 4, 4),
                "drive/edge_score": np.array([e["score"] for e in det.edges]),
                "drive/n_points": np.array([len(c) for c in det.clouds], np.int64)})
    print("drive: matchings", len(ms), "edges", out["drive/edges"].tolist(), "scores", out["drive/edge_score"])
    for m in ms:
        print(" ", m["new_id"], m["candidates"], m["iterations"], [f"{s:.3g}" for s in m["score"]], "best", m["best"], "fine", m["fine"][1:] if m["fine"] else None)
    path = os.path.join(ROOT, "tests", "golden", "loop.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
