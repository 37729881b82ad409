"""A/B of the large-scan fp16 first pass with and without the resident fp16 image, one process, one
handle: the synthetic matrix of bench.py's hbm_scan (10 M x 768 by default), the two forms run ALTERNATELY by toggling
AMDR_DENSE_HI_IMAGE per window, device events around enough searches for a window of >= AB_WINDOW_S seconds after a
warm-up, 5 windows per form.  Prints one JSON line per case: build time and bytes of the image, median / min / max ms per
search of both forms, the fraction of 8 TB/s the image form reaches on its first-pass bytes, and `pass`: the image
form's median lies below the image-less form's fastest window.  Ids of the two forms are asserted equal on every
timed search.

  AB_N, AB_D, AB_CASES="64:10,8:10,32:10" (queries:k), AB_WINDOWS=5, AB_WINDOW_S=0.5"""
import json
import os
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from legal_rag_amd import _native  # noqa: E402

HBM_PEAK = 8.0e12


def window(idx, Q, B, k, s, i, searches, image, ref_ids):
    os.environ["AMDR_DENSE_HI_IMAGE"] = "1" if image else "0"
    st = int(torch.cuda.current_stream().cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    same = torch.ones((), dtype=torch.bool, device=Q.device)
    e0.record()
    for _ in range(searches):
        idx.search_device(Q.data_ptr(), B, k, s.data_ptr(), i.data_ptr(), st)
        if ref_ids is not None:
            same &= (i == ref_ids).all()
    e1.record()
    torch.cuda.synchronize()
    assert bool(same), f"ids differ between the forms (image={image}, B={B}, k={k})"
    return e0.elapsed_time(e1) / searches


def main():
    n = int(os.environ.get("AB_N", 10_000_000))
    d = int(os.environ.get("AB_D", 768))
    windows = int(os.environ.get("AB_WINDOWS", 5))
    window_s = float(os.environ.get("AB_WINDOW_S", 0.5))
    dev = torch.device("cuda:0")
    X = bench.synth_matrix(torch, n, d, dev, seed=1234)
    Q = bench.synth_queries(torch, dev)
    if d != 768:
        Q = torch.nn.functional.normalize(torch.randn(1024, d, device=dev, generator=torch.Generator(dev).manual_seed(5)), dim=1)
    idx = _native.DenseIndex(device_ptr=X.data_ptr(), n=n, dim=d, device=0, keepalive=X)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx.build_image()
    build_s = time.perf_counter() - t0
    present, img_bytes, rows, e = idx.image_info()
    assert present and rows == n
    cases = [tuple(int(v) for v in c.split(":")) for c in os.environ.get("AB_CASES", "64:10,8:10,32:10").split(",")]
    for B, k in cases:
        idx.reserve(B, k)
        s = torch.empty((B, k), dtype=torch.float32, device=dev)
        i = torch.empty((B, k), dtype=torch.int64, device=dev)
        plans = {}
        for image in (False, True):
            os.environ["AMDR_DENSE_HI_IMAGE"] = "1" if image else "0"
            plans[image] = idx.plan_info(B, k)[:48]
        # the reference ids (image-less form) and the warm-up of both forms; the window length from the slower form
        ms0 = window(idx, Q, B, k, s, i, 3, False, None)
        ref = i.clone()
        window(idx, Q, B, k, s, i, 3, True, ref)
        searches = max(3, int(window_s * 1e3 / ms0) + 1)
        t = {False: [], True: []}
        for _ in range(windows):
            for image in (False, True):
                t[image].append(window(idx, Q, B, k, s, i, searches, image, ref))
        med = {f: sorted(v)[len(v) // 2] for f, v in t.items()}
        # the first pass reads the image twice per search: the strided sample (a fraction) and the full scan
        out = {"n": n, "d": d, "queries": B, "k": k, "image_bytes": img_bytes, "image_build_s": round(build_s, 3),
               "scale_exp": e, "searches_per_window": searches, "windows": windows,
               "plain": {"plan": plans[False], "median_ms": med[False], "min_ms": min(t[False]), "max_ms": max(t[False])},
               "image": {"plan": plans[True], "median_ms": med[True], "min_ms": min(t[True]), "max_ms": max(t[True])},
               "image_search_fraction_of_8TBs": img_bytes / (med[True] * 1e-3) / HBM_PEAK,
               "pass": med[True] < min(t[False]), "ids_equal": True, "counters": list(idx.hi_counters())}
        print(json.dumps(out), flush=True)
    idx.close()


if __name__ == "__main__":
    main()
