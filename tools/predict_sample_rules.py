#!/usr/bin/env python3
"""tools/predict_sample_rules.py - what k_predict's table makes of a frame under different rules for the sampled line's place in its group
(csrc/ssd_predict.h: predict_sample_offset).  CPU only: the frames of the benchmark from the host generator, every point a rule does not
sample blanked, the oracle's complete histogram of the rest = the kernel's sample (tests/test_gpu_predict_sample.py holds the kernel to
exactly that), the host statement of the table on it.

    python tools/predict_sample_rules.py planes xga [every]     planes per frame on the bench's 1024 XGA frames (every n-th; default all)
    python tools/predict_sample_rules.py planes fhd [every]     the same on the 256 frames of FHD stress
    python tools/predict_sample_rules.py widths                 widths 256 .. 2048 at 4:3 where a band of 64 columns leaves 0.75 .. 1.25 of its share

Rules: `runs16` = the parent's (one run of 16 points of every 16 runs, at (g * 5) & 15); `k/<d>` = whole lines, the place
floor(15 frac(g c)) with c = (golden ratio - 1) / d (d = 1: the golden ratio itself), `hash` = a hash of g.  profiles/predict_whole_lines.txt
holds the output."""
import importlib
import os
import sys
from multiprocessing import Pool

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
PHI = 0.6180339887498949
DIVISORS = (1, 8, 28, 40, 44, 48, 52, 56, 64)


def creep(d):
    a = int(PHI / d * 2 ** 32)
    return lambda g: ((((g * a) & 0xffffffff) >> 16) * 15) >> 16


def hashed(g):
    h = (g * 0x85EBCA6B) & 0xffffffff
    h = (((h >> 13) ^ h) * 0xC2B2AE35) & 0xffffffff
    return ((h >> 16) * 15) >> 16


def sampled_lines(n, off):
    """indices of the points of an aligned frame of n points that lie in the sampled lines"""
    groups = ((12 * n + 127) // 128 + 14) // 15
    g = np.arange(groups, dtype=np.int64)
    lo = (15 * g + off(g)) * 128
    idx = ((lo + 11) // 12)[:, None] + np.arange(10)[None, :]
    idx = idx[(12 * idx + 12 <= (lo + 128)[:, None]) & (idx < n)]
    return idx


def sampled_runs16(n):
    runs = n // 16
    g = np.arange((runs + 15) // 16, dtype=np.int64)
    run = g * 16 + ((g * 5) & 15)
    idx = (run[run < runs] * 16)[:, None] + np.arange(16)[None, :]
    return idx.ravel()


def rules(n):
    out = {"runs16": sampled_runs16(n), "hash": sampled_lines(n, hashed)}
    for d in DIVISORS:
        out["k/%d" % d] = sampled_lines(n, creep(d))
    return out


def _planes(job):
    fhd, ids = job
    ssd = importlib.import_module("stair-step-detector_amd")
    import oracle_binding as ob
    import scenes
    W, H = (1920, 1080) if fhd else (1024, 768)
    sc = scenes.fhd_stress_scenes(ssd, 256, base_seed=9000) if fhd else scenes.batch_scenes(ssd, W, H, 1024, base_seed=100000, rng_seed=1000)
    trans, cfg = ssd.transformation_for_scene(sc[0]), ssd.default_config(W, H)
    oc, ocal = ob.to_oracle_config(cfg), ob.to_oracle_calibration(trans.constants)
    oracle = ob.load_oracle()
    masks = {}
    for name, idx in rules(W * H).items():
        masks[name] = np.zeros(W * H, dtype=bool)
        masks[name][idx] = True
    out = []
    for i in ids:
        x = ssd.synth_host([sc[i]])[0]
        full = oracle.process(oc, ocal, x, images=0, ground_images=False)[0]
        row = {"full/16": ssd.predict_table_host(np.array(full.hist[:ssd.MAX_BINS], dtype=np.uint32) // 16, full.n_bins, full.min_height)[1]}
        for name, m in masks.items():
            c = x.reshape(-1, 3).copy()
            c[~m] = 0.0
            r = oracle.process(oc, ocal, c.reshape(H, W, 3), images=0, ground_images=False)[0]
            row[name] = ssd.predict_table_host(np.array(r.hist[:ssd.MAX_BINS], dtype=np.uint32), full.n_bins, full.min_height)[1]
        out.append(row)
    return out


def planes(fhd, every):
    ids = list(range(0, 256 if fhd else 1024, every))
    with Pool(8) as pool:
        rows = sum(pool.map(_planes, [(fhd, ids[k::8]) for k in range(8)]), [])
    print("%s, %d frames: planes per frame by the rule of the sampled line's place" % ("FHD stress" if fhd else "XGA bench batch", len(rows)))
    for name in rows[0]:
        print("  %-8s %.3f" % (name, np.mean([r[name] for r in rows])))


def widths():
    for d in DIVISORS:
        bad = []
        for W in range(256, 2049):
            idx = sampled_lines(W * (W * 3 // 4), creep(d))
            bands = (W + 63) // 64
            got = np.bincount((idx % W) // 64, minlength=bands)
            ratio = got / (len(idx) * np.minimum(64, W - 64 * np.arange(bands)) / W)
            if ratio.min() < 0.75 or ratio.max() > 1.25:
                bad.append(W)
        print("k/%-3d %2d of 1793 widths: %s" % (d, len(bad), " ".join(str(w) for w in bad)))


if __name__ == "__main__":
    if sys.argv[1] == "widths":
        widths()
    else:
        planes(sys.argv[2] == "fhd", int(sys.argv[3]) if len(sys.argv) > 3 else 1)
