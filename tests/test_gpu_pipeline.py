"""GPU parity of the whole hot path (zero_fill -> apodize_exp -> to_spectrum -> autophase) against the
CPU oracle, on the reference's quick-start shape and on synthetic multi-voxel FIDs.

Parity contract (DESIGN.md "Parity"):
  (i)   arg-max flat index, target index and pivot: exact;
  (ii)  with the oracle's (p0, p1) injected, the phased spectra match to <= 1e-5 of the max (c64)
        / 1e-12 (c128)  -- this is the data-parallel path proper;
  (iii) the host solver (same scipy differential evolution, same seed, same objective arithmetic) runs
        on the arg-max spectrum recomputed in complex128 on the device, so it reproduces the oracle's
        (p0, p1) for both storage precisions on structured signals; on the README's pure-noise input the
        ACME landscape is flat and 1e-16 differences move the polished optimum by ~1e-4 degrees.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = {"complex64": 1e-5, "complex128": 1e-12}


@pytest.fixture(scope="module")
def mods():
    import torch

    from xmris_amd import device, pipeline

    assert torch.cuda.is_available()
    return device, pipeline


def _relerr(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _three_peak(nv, nt, dt, seed=42, sigma=0.02):
    t = np.arange(nt) * dt
    amps, damps, freqs = (1.0, 0.5, 0.3), (20.0, 33.0, 25.0), (300.0, -800.0, 1100.0)
    base = sum(a * np.exp(-d * t) * np.exp(2j * np.pi * f * t) for a, d, f in zip(amps, damps, freqs))
    rng = np.random.default_rng(seed)
    amp = 0.5 + (np.arange(nv) % 997) / 997.0
    amp[nv // 3] = 2.0
    x = amp[:, None] * base[None, :] + sigma * (rng.standard_normal((nv, nt)) + 1j * rng.standard_normal((nv, nt))) / np.sqrt(2)
    return x, t


def _late_burst(t, amp, f0=650.0, lo=600, hi=1000):
    """A row whose signal starts after the samples either guess stage looks at (the coarse spectra read samples
    0...511, the L1 subset block 0 of every eight 128-sample blocks): the tallest peak of its dataset, invisible to
    the guess -> the verification must catch it."""
    burst = np.zeros(len(t), dtype=np.complex128)
    burst[lo:hi] = amp * np.exp(2j * np.pi * f0 * t[lo:hi])
    return burst


def _guess_kind(monkeypatch, kind):
    if kind == "l1":
        monkeypatch.setenv("XM_GUESS_L1", "1")  # round 2's guess: the windowed L1 norm's winner, no candidates
    else:
        monkeypatch.delenv("XM_GUESS_L1", raising=False)


def _check(mods, oracle, x, t, target, lb, dtype, dp_tol=1e-9):
    dev, pipe = mods
    xs = x.astype(dtype)
    ref, info = oracle.pipeline_values(xs.astype(np.complex128), t, target, lb, peak_width=100)
    xd = dev.to_device(xs)
    # (ii) oracle's parameters injected
    out, res, plan = pipe.run(xd, t, target, lb, params=(info["p0"], info["p1"]))
    assert res.flat_index == info["flat_idx"]
    assert res.target_idx == info["target_idx"]
    assert res.pivot == info["pivot"]
    np.testing.assert_array_equal(plan.freq, info["freq"])
    assert _relerr(out.cpu().numpy(), ref) < TOL[dtype]
    # (iii) own solve
    out2, res2, _ = pipe.run(xd, t, target, lb)
    assert res2.flat_index == info["flat_idx"] and res2.pivot == info["pivot"]
    f_mine = oracle.acme_score([res2.p0, res2.p1], info["slice"], info["freq"], info["pivot"])
    f_ref = oracle.acme_score([info["p0"], info["p1"]], info["slice"], info["freq"], info["pivot"])
    dp = (abs(res2.p0 - info["p0"]), abs(res2.p1 - info["p1"]))
    print(f"\n[{dtype}] oracle (p0,p1)=({info['p0']:.6f},{info['p1']:.6f}) nfev={info['nfev']}  "
          f"device-path (p0,p1)=({res2.p0:.6f},{res2.p1:.6f}) nfev={res2.nfev}  |dp|={dp}  "
          f"f_ref={f_ref:.12g} f_mine={f_mine:.12g}")
    assert dp[0] < dp_tol and dp[1] < dp_tol
    assert f_mine <= f_ref + 1e-6 * abs(f_ref)
    # Round 4: the search runs on the reference's slice bit for bit (the winning row's spectrum is computed with the
    # reference's numpy statements, `pipeline.winner_spectrum`), its generations replicate scipy's and its polish
    # follows scipy's route -- so (p0, p1) ARE the oracle's (measured: |dp| = 0.0 exactly on every config, the flat
    # landscape of the README's noise included; rounds 1-3: 3e-6 ... 2e-5 of the spectrum's maximum there) and the
    # phased spectra sit at the storage-precision floor: 1e-14 complex128, 2e-7 complex64 (profiles/r04/c1_tolerance.txt)
    assert _relerr(out2.cpu().numpy(), ref) < (1e-6 if dtype == "complex64" else 1e-12)
    np.testing.assert_allclose(np.abs(out2.cpu().numpy()), np.abs(ref), rtol=0, atol=2e-6 * np.abs(ref).max()
                               if dtype == "complex64" else 1e-12 * np.abs(ref).max())
    return dp


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_c1_readme_quickstart(mods, oracle, dtype):
    """BASELINE configs[0]: 5 voxels x 1024 noise FID, zero_fill(2048), lb=5 (README.md:55-73)."""
    rng = np.random.default_rng(42)
    t = np.linspace(0, 1, 1024)
    x = rng.standard_normal((5, 1024)) + 1j * rng.standard_normal((5, 1024))
    _check(mods, oracle, x, t, 2048, 5.0, dtype)  # pure noise, a flat objective: (p0, p1) still equal the oracle's


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_streaming_executor_returns_the_oracles_parameters(mods, oracle, dtype):
    """`run_stream(speculate=True)` -- the executor `bench.py` times -- over eight DISTINCT datasets (own noise, the
    brightest voxel somewhere else each time, two of them noise only, one guessed wrong and repaired): every dataset's
    (p0, p1), pivot and flat index equal the CPU oracle's on the same array (|dp| < 1e-9 degrees; the search runs on the
    reference's slice bit for bit) and every phased spectrum sits at the storage floor."""
    import torch

    dev, pipe = mods
    nv, nt, target = 64, 1024, 2048
    sets = []
    for k in range(8):
        x, t = _three_peak(nv, nt, 2e-4, seed=300 + k)
        x[(7 * k + 3) % nv] *= 1.7
        if k in (2, 5):  # noise only: the flat landscape
            rng = np.random.default_rng(900 + k)
            x = rng.standard_normal((nv, nt)) + 1j * rng.standard_normal((nv, nt))
        if k == 6:  # a late burst: invisible to the coarse spectra, the tallest line of the dataset -> repaired
            x[11] = _late_burst(t, 60.0)
        sets.append(x.astype(dtype))
    refs = [oracle.pipeline_values(x, t, target, 5.0, peak_width=100) for x in sets]
    xd = [dev.to_device(x) for x in sets]
    plan = pipe.make_plan(xd[0], t, target, 5.0)
    outs = [torch.empty((nv, target), dtype=xd[0].dtype, device="cuda") for _ in sets]
    got = pipe.run_stream(xd, outs, plan, speculate=True)
    torch.cuda.synchronize()
    assert [r.speculation for r in got] == ["repaired" if k == 6 else "hit" for k in range(8)]
    for k, (r, (ref, info)) in enumerate(zip(got, refs)):
        assert (r.flat_index, r.pivot) == (info["flat_idx"], info["pivot"]), k
        assert abs(r.p0 - info["p0"]) < 1e-9 and abs(r.p1 - info["p1"]) < 1e-9, (k, r.p0 - info["p0"], r.p1 - info["p1"])
        assert _relerr(outs[k].cpu().numpy(), ref) < (1e-6 if dtype == "complex64" else 1e-12), k


def test_autophase_parameters_are_the_oracles_on_random_datasets():
    """`tests/tool_sweep_autophase_exact.py` (seed 0, 14 datasets of its five families -- a few lines, many lines, noise only, one
    voxel far brighter, short FIDs incl. chirp-z lengths and no zero fill -- in both storage precisions): (p0, p1) of
    the fused path are the CPU oracle's on the same array (|dp| < 1e-9 degrees; measured: exactly equal in 80 of 80,
    profiles/r04/autophase_exact_sweep.txt) and the phased spectra sit at the storage floor.  Reference statement served:
    phasing.py:229-290 end to end."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "tool_sweep_autophase_exact.py"), "0", "14"], cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("case")]
    assert len(lines) == 28
    for ln in lines:
        dp = float(ln.split("|dp|")[1].split()[0])
        err = float(ln.split("spectrum rel err")[1].split()[0])
        assert dp < 1e-9, ln
        assert err < (1e-12 if "complex128" in ln else 1e-6), ln
    print(r.stdout.splitlines()[-1])


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_c2_shaped_grid(mods, oracle, dtype):
    """BASELINE configs[1]-shaped: 4x4x4 voxels x 2048 -> 4096 (grid flattened by the host layer)."""
    x, t = _three_peak(64, 2048, 1 / 5000.0)
    _check(mods, oracle, x, t, 4096, 5.0, dtype)


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_c3_shaped_small(mods, oracle, dtype):
    """BASELINE configs[2]-shaped, few voxels: 48 x 4096 -> 8192 through the persistent kernel."""
    x, t = _three_peak(48, 4096, 1 / 5000.0)
    _check(mods, oracle, x, t, 8192, 5.0, dtype)


def test_c5_mixed_radix_no_zero_fill(mods, oracle):
    """BASELINE configs[4]-shaped: 8 coils x 4 x 4 voxels x 1536-pt FID, no zero fill (2^9 * 3)."""
    x, t = _three_peak(128, 1536, 1 / 5000.0)
    _check(mods, oracle, x, t, 1536, 5.0, "complex64")


def test_full_size_properties(mods, oracle):
    """BASELINE configs[2] at full size (65,536 x 4096 -> 8192, c64): size-independent checks --
    the designated brightest voxel wins the global arg-max, |out| is unchanged by the phase,
    Parseval holds per spectrum, and a sample of rows matches the oracle."""
    import torch

    dev, pipe = mods
    nv, nt, N = 65536, 4096, 8192
    dt = 1 / 5000.0
    t = np.arange(nt) * dt
    base = sum(a * np.exp(-d * t) * np.exp(2j * np.pi * f * t)
               for a, d, f in zip((1.0, 0.5, 0.3), (20.0, 33.0, 25.0), (300.0, -800.0, 1100.0)))
    g = torch.Generator(device="cuda").manual_seed(7)
    amp = 0.5 + torch.remainder(torch.arange(nv, device="cuda", dtype=torch.float64), 997.0) / 997.0
    star = nv // 3
    amp[star] = 2.0
    x = amp[:, None].float() * torch.from_numpy(base).to("cuda", torch.complex64)[None, :]
    x = x + torch.view_as_complex(torch.randn((nv, nt, 2), generator=g, device="cuda") * (0.02 / np.sqrt(2)))
    out, res, plan = pipe.run(x, t, N, 5.0)
    assert res.flat_index // N == star
    rows = [0, 1, star - 1, star, star + 1, nv - 1]
    xs = x[rows].cpu().numpy().astype(np.complex128)
    zf, _ = oracle.zero_fill_values(xs, 1, N, "end")
    spec = oracle.to_spectrum_values(zf * oracle.exp_window(plan.time, 5.0), 1)
    ref = oracle.phase_values(spec, plan.freq, 1, res.p0, res.p1, res.pivot)
    got = out[rows].cpu().numpy()
    assert _relerr(got, ref) < 1e-5
    assert res.target_idx == int(np.argmax(np.abs(spec[3])))
    # Parseval (ortho FFT): sum |X|^2 == sum |x w|^2 per spectrum, all rows, on the device
    e_out = (out.real.double() ** 2 + out.imag.double() ** 2).sum(dim=1)
    xw = x * plan.window[:nt][None, :]
    e_in = (xw.real.double() ** 2 + xw.imag.double() ** 2).sum(dim=1)
    assert float(((e_out - e_in).abs() / e_in).max()) < 1e-5


@pytest.mark.parametrize("overlap", [True, False])
def test_run_stream_equals_one_dataset_at_a_time(mods, overlap):
    """The software-pipelined executor (what bench.py times) must give, dataset by dataset, exactly what the
    one-shot `run` gives: same winner, same (p0, p1), same phased spectra -- with five DIFFERENT datasets in
    flight, so a mixed-up double buffer (pre-pass outputs, pinned selection buffers, phase tables) shows."""
    import torch

    dev, pipe = mods
    nv, nt, target = 96, 512, 1024
    sets, t = [], None
    for k in range(5):
        x, t = _three_peak(nv, nt, 2e-4, seed=100 + k)
        x[nv // 3] *= 0.2             # move the winner: a different row (and scale) per dataset
        x[(7 * k + 3) % nv] *= 3.0 + k
        sets.append(dev.to_device(x.astype(np.complex64)))
    plan = pipe.make_plan(sets[0], t, target, 5.0)
    outs = [torch.empty((nv, target), dtype=torch.complex64, device="cuda") for _ in sets]
    trace = []
    results = pipe.run_stream(sets, outs, plan, overlap=overlap, trace=trace)
    torch.cuda.synchronize()
    assert len(results) == len(trace) == 5
    for k, (xd, od, r) in enumerate(zip(sets, outs, results)):
        ref_out, ref_res, _ = pipe.run(xd, t, target, 5.0, polish="native")  # (run_stream polishes natively)
        assert (r.flat_index, r.target_idx, r.pivot) == (ref_res.flat_index, ref_res.target_idx, ref_res.pivot), k
        assert r.flat_index // target == (7 * k + 3) % nv
        assert (r.p0, r.p1) == (ref_res.p0, ref_res.p1), k
        assert torch.equal(od, ref_out), k
        assert trace[k]["pre0"].elapsed_time(trace[k]["main1"]) > 0


@pytest.mark.parametrize("kind", ["coarse", "l1"])
def test_run_stream_speculative_hits_and_repairs(mods, oracle, monkeypatch, kind):
    """[kind = "l1": round 2's guess stage; "coarse": the coarse-spectra candidates see through the thirty-line row and
    every dataset is a hit]  speculate=True guesses the winning row from the windowed L1 norms, verifies it against the true per-row
    maxima the main pass returns, and repairs a wrong guess in place.  Datasets 0-2: rows of one spectral shape
    (the guess is right); datasets 3-4: one row carries thirty unit resonances (largest L1 norm, peaks of height
    about one) while the global maximum sits in a row with a single line of height 2.5 -- the guess is wrong and must
    be repaired.  Either way
    every output equals the non-speculative result (same winner, same (p0, p1), spectra to one rounding)."""
    import torch

    dev, pipe = mods
    _guess_kind(monkeypatch, kind)
    nv, nt, target = 80, 1024, 2048
    t = np.arange(nt) * 2e-4
    sets = []
    for k in range(5):
        x, _ = _three_peak(nv, nt, 2e-4, seed=300 + k)
        x[nv // 3] *= 0.3
        x[(11 * k + 5) % nv] *= 2.5
        if k >= 3:  # thirty unit lines in one row: its L1 norm adds up (~5 single lines), its peaks do not
            x *= 0.05
            lines = np.random.default_rng(k).uniform(-2300.0, 2300.0, 30)
            x[7] = sum(np.exp(-20.0 * t) * np.exp(2j * np.pi * f0 * t) for f0 in lines)
            x[50] = 2.5 * np.exp(-20.0 * t) * np.exp(2j * np.pi * -400.0 * t)
        sets.append(dev.to_device(x.astype(np.complex64)))
    plan = pipe.make_plan(sets[0], t, target, 5.0)
    outs = [torch.empty((nv, target), dtype=torch.complex64, device="cuda") for _ in sets]
    ref_outs = [torch.empty_like(o) for o in outs]
    ref = pipe.run_stream(sets, ref_outs, plan)
    got = pipe.run_stream(sets, outs, plan, speculate=True)
    torch.cuda.synchronize()
    assert [r.speculation for r in got] == (["hit", "hit", "hit", "repaired", "repaired"] if kind == "l1" else ["hit"] * 5)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert (a.flat_index, a.target_idx, a.pivot) == (b.flat_index, b.target_idx, b.pivot), k
        assert (a.p0, a.p1) == (b.p0, b.p1), k
        scale = float(ref_outs[k].abs().max())
        # a hit applies the same (p0, p1) in a different instantiation of the kernel (with the per-row maxima): equal to
        # one rounding of the storage precision; a repair multiplies by the phase ratio afterwards (two more roundings)
        assert float((outs[k] - ref_outs[k]).abs().max()) < (1e-6 if a.speculation == "repaired" else 2.5e-7) * scale, k
    assert got[3].flat_index // target == 50


@pytest.mark.parametrize("kind", ["coarse", "l1"])
def test_speculative_guess_on_a_subset_misses_and_is_repaired(mods, monkeypatch, kind):
    """[kind = "coarse": the coarse spectra read samples 0...511 of a row, the burst sits in 600...999]
    The L1 guess kernel sums every 8th 1-KiB block (128 samples) of the leading samples only.  Row 9 of dataset 1 carries ALL its
    signal in blocks the guess skips (samples 128...511: a delayed burst), and the tallest peak of the dataset: the
    full L1 norm would find it, the subset cannot.  The verification must catch it and the repaired result must equal
    the classic schedule's; dataset 0 (ordinary decaying rows) is a hit."""
    import torch

    dev, pipe = mods
    _guess_kind(monkeypatch, kind)
    nv, nt, target = 48, 1024, 2048
    t = np.arange(nt) * 2e-4
    sets = []
    for k in range(2):
        x, _ = _three_peak(nv, nt, 2e-4, seed=500 + k)
        x[(5 * k + 2) % nv] *= 2.0
        if k == 1:
            if kind == "l1":
                burst = np.zeros(nt, dtype=np.complex128)
                burst[128:512] = 12.0 * np.exp(2j * np.pi * 650.0 * t[128:512])  # 384 samples of one frequency
            else:
                burst = _late_burst(t, 60.0)
            x[9] = burst
        sets.append(dev.to_device(x.astype(np.complex64)))
    plan = pipe.make_plan(sets[0], t, target, 5.0)
    outs = [torch.empty((nv, target), dtype=torch.complex64, device="cuda") for _ in sets]
    refs = [torch.empty_like(o) for o in outs]
    ref = pipe.run_stream(sets, refs, plan)
    got = pipe.run_stream(sets, outs, plan, speculate=True)
    torch.cuda.synchronize()
    assert ref[1].flat_index // target == 9, "the burst row must hold the global maximum"
    assert [r.speculation for r in got] == ["hit", "repaired"]
    for k, (a, b) in enumerate(zip(got, ref)):
        assert (a.flat_index, a.target_idx, a.pivot, a.p0, a.p1) == (b.flat_index, b.target_idx, b.pivot, b.p0, b.p1), k
        scale = float(refs[k].abs().max())
        assert float((outs[k] - refs[k]).abs().max()) < 1e-6 * scale, k


@pytest.mark.parametrize("dtype,nt,target", [("complex128", 1024, 2048), ("complex128", 4096, 8192), ("complex64", 1536, 1536),
                                             ("complex64", 1000, 2048), ("complex64", 8192, 16384),
                                             # no zero fill on k_fft2's plans: the arg-max key of its ramp mode (round 4)
                                             ("complex64", 2048, 2048), ("complex64", 768, 768), ("complex64", 6144, 6144)])
def test_speculative_schedule_on_the_table_and_per_row_paths(mods, dtype, nt, target):
    """The speculative schedule where the packed complex64 kernel does not apply: complex128 (`k_zf2<double>` /
    `k_zf2d` with the ramp, per-row maxima + reductions instead of arg-max keys) and no zero fill / mixed radix /
    unaligned rows (a phase table instead of the ramp) -- same results as the classic schedule, hits and a repair."""
    import torch

    dev, pipe = mods
    nv = 41 if nt == target else 40  # (an odd row count too: k_fft2 packs two rows per lane pair)
    t = np.arange(nt) * 2e-4
    sets = []
    for k in range(3):
        x, _ = _three_peak(nv, nt, 2e-4, seed=700 + k)
        x[(3 * k + 1) % nv] *= 2.0
        if k == 2:  # a late burst: the tallest peak of the dataset in samples no guess stage reads
            x[20] = _late_burst(t, 60.0)
        sets.append(dev.to_device(x.astype(dtype)))
    plan = pipe.make_plan(sets[0], t, target, 5.0)
    outs = [torch.empty((nv, target), dtype=sets[0].dtype, device="cuda") for _ in sets]
    refs = [torch.empty_like(o) for o in outs]
    ref = pipe.run_stream(sets, refs, plan)
    got = pipe.run_stream(sets, outs, plan, speculate=True)
    torch.cuda.synchronize()
    assert [r.speculation for r in got] == ["hit", "hit", "repaired"] and got[2].flat_index // target == 20
    for k, (a, b) in enumerate(zip(got, ref)):
        assert (a.flat_index, a.target_idx, a.pivot, a.p0, a.p1) == (b.flat_index, b.target_idx, b.pivot, b.p0, b.p1), k
        tol = 2.5e-7 if dtype == "complex64" else 1e-14
        assert float((outs[k] - refs[k]).abs().max()) <= tol * float(refs[k].abs().max()), k


def test_bench_self_launches_two_ranks():
    """`python bench.py --gpus 2` without a launcher must start two rank processes itself (sharing this GPU here, gloo
    instead of RCCL) and report n_gpus == 2; with one visible device and no --share-gpu it must refuse (exit != 0)
    instead of quietly benchmarking one rank."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    # with the wall-clock priming loop on: every rank must leave it after the same number of calls (each call is a
    # sequence of exchanges; ranks that read their own clocks ended up one call apart and deadlocked)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--share-gpu", "--dist-backend", "gloo", "--steps", "3",
           "--warmup", "1", "--voxels", "2048", "--no-cpu-baseline", "--prime-ms", "60"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["value"] > 0 and rec["config"]["voxels_per_gpu"] == 2048
    import torch

    if torch.cuda.device_count() < 2:
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2"], cwd=root, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "device(s) visible" in r.stderr


def test_bench_plain_run_dumps_the_last_step(tmp_path):
    """A plain `bench.py` run measures the headline alone (no `--full` record in its line), reports the steps it was
    given, and `--dump-outputs` writes the last timed step's outputs: float arrays within 64 MB, the winner's spectrum
    peaking where the arg-max says, and the same arrays from a second run with the same arguments."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
               "--voxels", "4096", "--prime-ms", "0", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        rec = json.loads(lines[0])
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["dtype"] == "f32"
        for key in ("cpu_baseline", "cpu_baseline_all_cores", "parity", "configs", "c128", "heterogeneous",
                    "speculation_miss", "value_classic_schedule"):
            assert key not in rec, key
        names = sorted(os.listdir(d))
        assert names == ["autophase.npy", "spectra_sample.npy", "spectra_sample_rows.npy", "spectrum_winner.npy"]
        assert sum(os.path.getsize(d / n) for n in names) <= 64 << 20
        arrs = {n[:-4]: np.load(d / n) for n in names}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert arrs["spectra_sample"].shape == (arrs["spectra_sample_rows"].size, 8192, 2)
        p0, p1, pivot, flat, target_idx, max_abs = arrs["autophase"]
        win = arrs["spectrum_winner"][..., 0] + 1j * arrs["spectrum_winner"][..., 1]
        assert abs(abs(win[int(flat) % 8192]) - max_abs) <= 1e-5 * max_abs
        assert np.abs(win).max() <= max_abs * (1 + 1e-5)
        dumps.append(arrs)
    for n, a in dumps[0].items():
        b = dumps[1][n]
        if n == "autophase" or n == "spectra_sample_rows":
            assert np.array_equal(a, b), n
        else:
            assert float(np.abs(a - b).max()) <= 2.5e-7 * float(np.abs(a).max()), n


def test_speculative_schedule_two_ranks_with_cross_rank_repair():
    """Two ranks (sharing this GPU, gloo + the shared-memory exchange) run run_stream(speculate=True) on shards of
    datasets whose L1-norm winner lives on rank 0 while the true maximum lives on rank 1: the verification
    exchange must detect it, the owner of the true row re-searches, every rank rotates its shard, and the gathered
    result must equal the single-process classic schedule (scripts/check_spec_multirank.py does the comparison)."""
    import os
    import socket
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "scripts", "check_spec_multirank.py")]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "multi-rank speculative run_stream: OK" in r.stdout


@pytest.mark.parametrize("engine", ["host", "device"])
def test_speculative_schedule_four_ranks_share_the_gpu(engine):
    """FOUR ranks (the GPU box allows six processes on its card: this one, the four, and one to spare) share the GPU and
    run run_stream(speculate=True) on shards of twelve datasets: winners rotating over ranks 1..3, rank 0 never an owner,
    two cross-rank repairs -- with the searches on the library's native host threads and as search kernels on reserved
    CUs.  scripts/check_spec_ranks.py asserts, on every rank, the one-rank classic result bit for bit ((p0, p1), pivot,
    flat index), the gathered spectra to 1e-6, and equal exchange / broadcast call counts across the ranks."""
    import os
    import socket
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, XMRIS_AMD_SEARCH=engine)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "scripts", "check_spec_ranks.py")]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "4-rank speculative run_stream" in r.stdout and ": OK" in r.stdout
    print(r.stdout[-1500:])


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_speculative_stream_of_many_small_datasets_with_misses(mods, dtype):
    """Fourteen small datasets in one call: the device period is far shorter than a search, so four searches are in
    flight (`_search_workers`), the ring of guess / selection slots wraps twice, verifications lag two datasets and
    three of the datasets are built to be guessed wrong (repaired, one of them the very first, one the last).  Every
    (p0, p1, pivot, flat index) and every spectrum must equal the classic schedule's."""
    import torch

    dev, pipe = mods
    nv, nt, target = 96, 1024, 2048
    t = np.arange(nt) * 2e-4
    sets, wrong = [], {0, 6, 13}
    for k in range(14):
        x, _ = _three_peak(nv, nt, 2e-4, seed=900 + k)
        x[(5 * k + 2) % nv] *= 2.0
        if k in wrong:  # a late burst: the tallest peak of the dataset in samples no guess stage reads
            x[20 + k] = _late_burst(t, 60.0)
        sets.append(dev.to_device(x.astype(dtype)))
    plan = pipe.make_plan(sets[0], t, target, 5.0)
    assert pipe._search_workers(plan, nv, sets[0].element_size(), 8)[0] == 4
    outs = [torch.empty((nv, target), dtype=sets[0].dtype, device="cuda") for _ in sets]
    refs = [torch.empty_like(o) for o in outs]
    ref = pipe.run_stream(sets, refs, plan)
    got = pipe.run_stream(sets, outs, plan, speculate=True)
    torch.cuda.synchronize()
    assert [r.speculation for r in got] == ["repaired" if k in wrong else "hit" for k in range(14)]
    for k, (a, b) in enumerate(zip(got, ref)):
        assert (a.flat_index, a.target_idx, a.pivot, a.p0, a.p1) == (b.flat_index, b.target_idx, b.pivot, b.p0, b.p1), k
        tol = 2.5e-7 if dtype == "complex64" else 1e-14
        assert float((outs[k] - refs[k]).abs().max()) <= tol * float(refs[k].abs().max()), k


def test_a_search_that_runs_late_is_started_a_second_time(mods, monkeypatch):
    """`run_stream(speculate=True)` hedges a search whose thread lost its CPU: with the test hook that puts the search
    thread of dataset 9 to sleep for 40 ms, the launch thread has the same search started again once it is later than
    twice the typical run time and takes whichever ends first -- the result is the classic schedule's to the bit
    (the search is a pure function of the slice), only that dataset is flagged, and the call does not wait out the nap."""
    import time

    import torch

    dev, pipe = mods
    nv, nt, target = 96, 1024, 2048
    t = np.arange(nt) * 2e-4
    sets = []
    for k in range(14):
        x, _ = _three_peak(nv, nt, 2e-4, seed=700 + k)
        x[(7 * k + 3) % nv] *= 2.0
        sets.append(dev.to_device(x.astype("complex64")))
    plan = pipe.make_plan(sets[0], t, target, 5.0)
    outs = [torch.empty((nv, target), dtype=sets[0].dtype, device="cuda") for _ in sets]
    refs = [torch.empty_like(o) for o in outs]
    ref = pipe.run_stream(sets, refs, plan)
    pipe.run_stream(sets, outs, plan, speculate=True)  # warm: pools, plans
    monkeypatch.setenv("XM_TEST_SLOW_SEARCH", "9,40")
    for attempt in range(3):  # (a busy host may hedge an earlier dataset of its own accord: at most one in eight)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = pipe.run_stream(sets, outs, plan, speculate=True)
        torch.cuda.synchronize()
        hedged_s = time.perf_counter() - t0
        if [k for k, r in enumerate(got) if r.hedged] == [9]:
            break
    assert [k for k, r in enumerate(got) if r.hedged] == [9]
    for k, (a, b) in enumerate(zip(got, ref)):
        assert (a.flat_index, a.target_idx, a.pivot, a.p0, a.p1) == (b.flat_index, b.target_idx, b.pivot, b.p0, b.p1), k
        assert float((outs[k] - refs[k]).abs().max()) <= 2.5e-7 * float(refs[k].abs().max()), k
    monkeypatch.setenv("XMRIS_AMD_HEDGE", "0")
    t0 = time.perf_counter()
    plain = pipe.run_stream(sets, outs, plan, speculate=True)
    torch.cuda.synchronize()
    waited_s = time.perf_counter() - t0
    assert not any(r.hedged for r in plain) and waited_s > 0.035  # without the hedge the nap is on the critical path
    assert hedged_s < waited_s - 0.015


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_speculative_schedule_on_an_all_zero_dataset(mods, dtype):
    """np.argmax of an all-zero array is 0 (phasing.py:229): the speculative schedule must guess row 0, verify row 0
    ("hit") and give the classic schedule's result -- the arg-max keys carry the row even when every |X|^2 is +0.0
    (round 2 published a key only for values above zero and crashed here).  A dataset of zeros sits between two
    ordinary ones."""
    import torch

    dev, pipe = mods
    nv, nt, target = 96, 4096, 8192
    t = np.arange(nt) * 2e-4
    a, _ = _three_peak(nv, nt, 2e-4, seed=11)
    sets = [dev.to_device(a.astype(dtype)), dev.to_device(np.zeros((nv, nt), dtype=dtype)), dev.to_device((2 * a).astype(dtype))]
    plan = pipe.make_plan(sets[0], t, target, 5.0)
    outs = [torch.empty((nv, target), dtype=sets[0].dtype, device="cuda") for _ in sets]
    refs = [torch.empty_like(o) for o in outs]
    ref = pipe.run_stream(sets, refs, plan)
    got = pipe.run_stream(sets, outs, plan, speculate=True)
    torch.cuda.synchronize()
    assert [r.speculation for r in got] == ["hit"] * 3 and got[1].flat_index == ref[1].flat_index == 0
    for k, (g, r) in enumerate(zip(got, ref)):
        assert (g.flat_index, g.target_idx, g.pivot) == (r.flat_index, r.target_idx, r.pivot), k
        if k != 1:
            assert (g.p0, g.p1) == (r.p0, r.p1), k
    assert float(outs[1].abs().max()) == 0.0


@pytest.mark.parametrize("dtype,nv", [("complex64", 8192), ("complex128", 4096)])
def test_speculative_schedule_hits_on_the_heterogeneous_family(mods, monkeypatch, dtype, nv):
    """bench.synth_hetero: per-voxel random line counts / widths / amplitudes, noise-only voxels and a lipid-like voxel
    with the largest windowed L1 norm.  The coarse-spectra guess stage must find the true arg-max voxel on every
    dataset ("hit") with the classic schedule's (p0, p1) and spectra; round 2's L1 guess misses at least one of them
    (repaired -- still the same results)."""
    import torch

    import bench

    dev, pipe = mods
    nt, target = 4096, 8192
    tdt = torch.complex64 if dtype == "complex64" else torch.complex128
    sets, lipids = [], []
    for seed in range(4):
        x, t, lip = bench.synth_hetero(torch, nv, nt, 2e-4, seed, "cuda", tdt)
        sets.append(x)
        lipids.append(lip)
    plan = pipe.make_plan(sets[0], t, target, 5.0)
    outs = [torch.empty((nv, target), dtype=tdt, device="cuda") for _ in range(2)]
    ref_out = torch.empty_like(outs[0])
    ref = [pipe.run_stream([x], [ref_out], plan)[0] for x in sets]
    got = pipe.run_stream(sets, [outs[k % 2] for k in range(4)], plan, speculate=True)
    torch.cuda.synchronize()
    assert [r.speculation for r in got] == ["hit"] * 4
    for k, (g, r) in enumerate(zip(got, ref)):
        assert (g.flat_index, g.target_idx, g.pivot, g.p0, g.p1) == (r.flat_index, r.target_idx, r.pivot, r.p0, r.p1), k
        assert g.flat_index // target != lipids[k]
    monkeypatch.setenv("XM_GUESS_L1", "1")
    old = pipe.run_stream(sets, [outs[k % 2] for k in range(4)], plan, speculate=True)
    torch.cuda.synchronize()
    assert "repaired" in [r.speculation for r in old]
    for k, (g, r) in enumerate(zip(old, ref)):
        assert (g.flat_index, g.p0, g.p1) == (r.flat_index, r.p0, r.p1), k
