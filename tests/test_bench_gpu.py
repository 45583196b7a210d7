"""bench.py's plain run on a small stream: the result line holds the headline fields and nothing that --full
measures, --steps sets the timed steps, and --dump-outputs writes the last step's tables: the key-hashed sample
of every rule must be exactly the oracle's rows under the same hash (sorted by key), the statistics and the
digest's row / pair totals the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import covis as oracle
import otto_recommender_amd.synth as synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVENTS = 300_000


def test_plain_run_line_and_dumped_tables(gpu, tmp_path):
    import bench
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--events", str(EVENTS), "--dump-outputs", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "pairs/s" and line["dtype"] == "int32"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert not {"phases_ms", "roofline", "phase_rooflines", "a6", "ingest", "cpu_baseline", "knn", "candidates"} & set(line)

    # the same stream on the host, file by file as bench.py generates it
    n_sess, _ = synth.sessions_for_events(EVENTS, 0, 0)
    fb = synth.file_session_bounds(n_sess)
    from otto_recommender_amd import config
    names = list(config.CO_EVENTS_TO_COUNT)  # the order of the table's rules, and of stats.npy's rows
    per_file = []
    for f in range(len(fb) - 1):
        ev = synth.generate(int(fb[f + 1] - fb[f]), int(fb[f]), 0)
        per_file += oracle.count_co_events_files(ev.session_offsets, ev.aid, ev.ts, ev.type,
                                                 np.array([0, ev.n_sessions], np.int64))
    thr = line["dump_outputs"]["sample_hash_below"]
    stats = np.load(os.path.join(out, "stats.npy"))
    total_rows, total_bytes = 0, 0
    for i, n in enumerate(names):
        ra = np.concatenate([p[n][0] for p in per_file]); rb = np.concatenate([p[n][1] for p in per_file])
        rc = np.concatenate([p[n][2] for p in per_file]).astype(np.int64)
        a, b, c = oracle._groupby_sum(ra, rb, rc)
        _, _, c2 = oracle._groupby_sum(ra, rb, np.where(rc >= 2, rc, 0))
        a, b = a.astype(np.int64), b.astype(np.int64)
        m = bench.sample_hash(a, b, 0) < thr
        ref = np.stack([a[m], b[m], c[m], c2[m]], 1)
        ref = ref[np.lexsort((ref[:, 1], ref[:, 0]))].astype(np.float64)
        got = np.load(os.path.join(out, f"{n}.npy"))
        assert got.dtype == np.float64 and np.array_equal(got, ref), n
        assert stats[i].tolist()[:2] == [len(a), int(c.sum())], n
        limbs = np.load(os.path.join(out, f"{n}_digest.npy")).astype(np.int64)
        val = [int(sum(int(x) << (16 * j) for j, x in enumerate(row))) for row in limbs]
        assert val[2] == int(c.sum()) and val[4] == len(a), n  # pairs, rows over the whole table
        total_rows += len(a)
    for f in os.listdir(out):
        total_bytes += os.path.getsize(os.path.join(out, f))
    assert thr < 1 << 32 and total_rows > bench.DUMP_SAMPLE_ROWS  # the sampling path ran, not the whole-table one
    assert total_bytes <= bench.DUMP_MAX_BYTES and len(os.listdir(out)) == 2 * len(names) + 1
