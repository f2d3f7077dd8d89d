"""Every record the device search's tests look at, into one .npz -- to compare two builds of csrc/xm_search.hip byte for
byte.  The cases of tests/_search_cases.py (`search_launch` without `seq` and `t_us`, `search_rows` on the same slice,
`search_eval` scores), and the inputs of tests/test_gpu_autophase_each.py (both lengths and dtypes, the FULL length, the
600-row hand-out, the pivot override with its degenerate rows).  The archive carries no time stamps: equal arrays give
equal files, and the script prints the file's SHA-256.

    python scripts/dump_search_records.py <out.npz>
"""
import hashlib
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def collect():
    import torch

    import _each_rows
    import _search_cases as sc
    from test_gpu_autophase_each import FULL_N, FULL_SEEDS, SEEDS
    from xmris_amd import device as dev

    shared = np.dtype([(f, sc.RESULT_DTYPE[f]) for f in sc.SHARED])
    out = {}
    rec = dev.new_search_record()
    for n, seed in sc.CASE_LIST:
        spec, freq, k = sc.make_slice(n, seed)
        axis = dev.uniform_axis(freq)
        pinned = torch.from_numpy(spec.copy()).pin_memory()
        xs = sc.eval_points(seed)
        out[f"eval_n{n}_s{seed}"] = dev.search_eval(pinned, axis, xs)
        out[f"eval_given_n{n}_s{seed}"] = dev.search_eval(pinned, axis, xs, target_idx=k)
        for p0_only in (False, True):
            sc.run_search(dev, pinned, axis, rec, sc.next_seq(), p0_only)
            full = rec.numpy().view(sc.RESULT_DTYPE)[0]
            single = np.zeros(1, shared)
            for f in sc.SHARED:
                single[f][0] = full[f]
            out[f"single_n{n}_s{seed}_p{int(p0_only)}"] = single
            out[f"rows_n{n}_s{seed}_p{int(p0_only)}"] = np.array([sc.rows_record(dev, spec, axis, k, p0_only)])
    for n, seeds, dtypes in ((512, SEEDS, ("complex128", "complex64")), (1000, SEEDS, ("complex128", "complex64")),
                             (FULL_N, FULL_SEEDS, ("complex128",))):
        rows, freq = _each_rows.make_rows(n, seeds)
        for dt in dtypes:
            out[f"each_n{n}_{dt}"] = dev.search_rows(dev.to_device(rows.astype(dt)), dev.uniform_axis(freq))
    rows, freq = _each_rows.make_rows(512, SEEDS)
    out["each_hand_out_600"] = dev.search_rows(dev.to_device(np.tile(rows, (50, 1))), dev.uniform_axis(freq))
    rows = rows[:4].copy()
    rows[1] = 0.0
    rows[3, 300] = complex(1.0, np.inf)
    tc = float(freq[200]) + 0.3 * float(freq[1] - freq[0])
    out["each_pivot_p0_only_degenerate"] = dev.search_rows(dev.to_device(rows), dev.uniform_axis(freq), p0_only=True, pivot=tc,
                                                           target_idx=int(np.argmin(np.abs(freq - tc))))
    return out


def write_npz(path, arrays):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            with z.open(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w") as fh:
                np.lib.format.write_array(fh, np.ascontiguousarray(arrays[name]), allow_pickle=False)
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


if __name__ == "__main__":
    digest = write_npz(sys.argv[1], collect())
    print(f"{digest}  {sys.argv[1]}")
