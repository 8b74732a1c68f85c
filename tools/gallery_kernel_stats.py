"""Kernel times of the gallery search (csrc/trl_gallery.hip) by the method of profiles/logits_kernel_stats.csv: rocprofv3 kernel
trace, one process per shape, median of 10 warm launches (after 10 of warm-up) and of 5 cold ones, each behind a 1 GiB fill.

    python tools/gallery_kernel_stats.py --all out_dir > profiles/gallery_kernel_stats.csv      # every shape, then the table
    rocprofv3 --kernel-trace -d out_dir/m_n -o t -f csv -- python3 tools/gallery_kernel_stats.py run M N     (what --all starts)
    python tools/gallery_kernel_stats.py --table out_dir

A launch's time is k_gallery_search plus k_gallery_merge.  Next to it: the two floors of the shape -- one pass over the gallery,
m * 2 KB at 8.0 TB/s, and 2 n 512 m FLOP at the 157.3 TFLOP/s f32-MFMA peak -- and what a user would
otherwise write on the same device: torch.mm(q, rows.T) + torch.topk(k), cosine on rows normalised beforehand (the sum of every
kernel the two calls launch, median of 10 after 10 of warm-up).

Cluster mode (FaceGallery.cluster: trl_cluster_links + trl_cluster_labels), n rows against themselves:

    python tools/gallery_kernel_stats.py --cluster out_dir > profiles/cluster_kernel_stats.csv
    python tools/gallery_kernel_stats.py --cluster-table out_dir

Per n one process under the same trace: 3 + 5 calls of cluster() (cosine 0.5, min_samples 4, on n / 16 identities of 16 noisy unit
rows each, so that there is a graph to label), then 3 + 5 of scores() on the same n x n -- k_gallery_scores, the kernel whose
main loop k_gallery_links shares, is the yardstick.  A row of the table is one kernel: its launches per call and the median over the
5 measured calls of its time per call (the label kernels run once per round).

Cluster-lists mode (FaceGallery.cluster(method="lists"): range_search() + trl_cluster_labels_lists), the same planted clusters:

    python tools/gallery_kernel_stats.py --cluster-lists out_dir > profiles/cluster_lists_kernel_stats.csv
    python tools/gallery_kernel_stats.py --cluster-lists-table out_dir

Per n (the cluster mode's and 131,072) and per density -- 16 rows an identity (mean degree 16), 128 and 1,024 -- one process under the same
trace: 3 + 5 calls of range_search() at cosine 0.5 (the two passes, the row sums and the scan); then, per forced lanes_per_row 4 / 16
/ 64, 3 + 5 calls of trl_cluster_labels_lists at min_samples 4 on those lists; then, where the bitmap fits (n <= 65,536), 3 + 5 calls
of cluster(method="bitmap"), whose labels must equal the lists'.  A row of the table is one kernel of one phase: its launches per
call and the median over the 5 measured calls of its time per call (the hook kernels run once per round).  The auto choice of
lanes_per_row (cl_list_lanes, csrc/trl_cluster.hip) is read from this table.

Histogram mode (FaceGallery.score_histogram: trl_gallery_hist), the same embeddings, labels = the identities, E = 1000 edges:

    python tools/gallery_kernel_stats.py --hist out_dir > profiles/hist_kernel_stats.csv
    python tools/gallery_kernel_stats.py --hist-table out_dir

Per n one process under the same trace, 3 + 5 calls of each phase in turn: score_histogram(rows, labels) (ALL pairs) followed by
score_histogram() (UPPER: each unordered pair once); cluster() and scores() as above -- k_gallery_links and k_gallery_scores of the
same run are the yardsticks; and, where the matrix fits (n <= 8192), what a user would otherwise write: scores() + torch.bucketize
+ torch.bincount (every kernel the three launch, k_gallery_scores included), whose counts must equal the histogram's.

Range mode (FaceGallery.range_search: trl_gallery_range_count + trl_gallery_range_fill), the same embeddings:

    python tools/gallery_kernel_stats.py --range out_dir > profiles/range_kernel_stats.csv
    python tools/gallery_kernel_stats.py --range-table out_dir

Per shape one process under the same trace -- n = m in self mode (range_search(), the gallery against itself) and 256 of the rows as
queries against 1,000,000 -- and in it 3 + 5 rounds, each round every phase once: range_search at cosine 0.5 (about 15 hits a row),
at the smallest shape also at -2 (every pair), cluster() where n = m (k_gallery_links, the same main loop as pass 1) and scores()
where the matrix is at most 2 GiB.  Then, where n <= 8192, what a user would otherwise write: scores() + a comparison + torch.nonzero
(every kernel they launch), whose lists must equal the range search's.  A row of the table is one kernel of one phase: the median
over the 5 measured rounds, the smallest and the largest.

Groups mode (FaceGallery.search_identities: trl_gallery_search_groups), the search's shapes, k = 1, 5, 16:

    python tools/gallery_kernel_stats.py --groups out_dir > profiles/groups_kernel_stats.csv
    python tools/gallery_kernel_stats.py --groups-table out_dir

Per shape one process under the same trace.  The gallery is m / 8 identities of 8 noisy unit rows each, shuffled; the queries are
noisy copies of n of the identities, so every query has eight strong matches of one group.  3 + 5 rounds, each round per k: search()
(k_gallery_search + k_gallery_merge: the yardstick, the same main loop), then trl_gallery_search_groups with all ids distinct (whose
result must equal the search's) and with the identities as ids (k_gallery_search_groups + k_gallery_merge_groups).  A row of the table
is one of the three at one k: the median over the 5 measured rounds of search + merge, the merge's share, and the ratio to the plain
search of the same rounds."""
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M_SHAPES, N_SHAPES, K = (1_000, 100_000, 1_000_000), (1, 32, 256), 5
HBM_BYTES_PER_US, MFMA_FLOP_PER_US = 8.0e6, 157.3e6
WARMUP, WARM, COLD = 10, 10, 5


def run(m, n):
    import torch
    from truely_amd.gallery import FaceGallery
    gen = torch.Generator(device="cuda").manual_seed(m + n)
    rows = torch.nn.functional.normalize(torch.randn((m, 512), generator=gen, device="cuda"), dim=1)
    q = torch.nn.functional.normalize(torch.randn((n, 512), generator=gen, device="cuda"), dim=1)
    gal = FaceGallery(metric="cosine", capacity=m)
    gal.add(rows, range(m))
    torch.cuda.synchronize()
    for _ in range(WARMUP + WARM):
        idx, score = gal.search(q, k=K)
    torch.cuda.synchronize()
    for _ in range(WARMUP + WARM):
        v, i = torch.topk(torch.mm(q, rows.t()), K, dim=1)
    torch.cuda.synchronize()
    big = torch.empty((1 << 30,), dtype=torch.uint8, device="cuda")
    for c in range(COLD):
        big.fill_(c)
        gal.search(q, k=K)
    torch.cuda.synchronize()
    same = float((i == idx).float().mean())                   # (float32 sums in another order: near-ties may swap)
    print(json.dumps({"m": m, "n": n, "workspace_bytes": int(gal.lib.trl_gallery_search_workspace(n, m, K, 0)), "torch_agreement": same}))


def _trace(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    return sorted(rows)


def table(out):
    print("m,n,k,metric,state,launches,median_us,min_us,max_us,merge_median_us,workspace_bytes,floor_hbm_us,floor_mfma_us,torch_mm_topk_median_us")
    for m in M_SHAPES:
        for n in N_SHAPES:
            d = os.path.join(out, f"{m}_{n}")
            info = json.load(open(os.path.join(d, "info.json")))
            tr = _trace(d)
            first = next(i for i, r in enumerate(tr) if "k_gallery_search" in r[2])
            tr = tr[first:]                                   # (behind the enrolment)
            launches, other = [], []                          # per search launch: [search ns, merge ns]; kernels between searches
            for s, e, name in tr:
                if "k_gallery_search" in name:
                    launches.append([e - s, 0])
                elif "k_gallery_merge" in name:
                    launches[-1][1] = e - s
                elif len(launches) == WARMUP + WARM:
                    other.append(e - s)
            assert len(launches) == WARMUP + WARM + COLD, len(launches)
            per = len(other) // (WARMUP + WARM)               # kernels of one mm + topk
            torch_us = statistics.median(sum(other[i * per:(i + 1) * per]) for i in range(WARMUP, WARMUP + WARM)) / 1e3
            hbm, mfma = m * 2048 / HBM_BYTES_PER_US, 2.0 * n * 512 * m / MFMA_FLOP_PER_US
            for state, part in (("warm", launches[WARMUP:WARMUP + WARM]), ("cold", launches[WARMUP + WARM:])):
                tot = [(a + b) / 1e3 for a, b in part]
                print(f"{m},{n},{K},cosine,{state},{len(part)},{statistics.median(tot):.1f},{min(tot):.1f},{max(tot):.1f},"
                      f"{statistics.median(b for _a, b in part) / 1e3:.1f},{info['workspace_bytes']},{hbm:.1f},{mfma:.1f},{torch_us:.1f}")


CL_SHAPES, CL_WARMUP, CL_WARM, CL_PER_ID = (1_024, 8_192, 32_768), 3, 5, 16
CL_KERNELS = ("k_gallery_links", "k_cluster_degree", "k_cluster_init", "k_cluster_hook", "k_cluster_jump", "k_cluster_number",
              "k_cluster_assign", "k_gallery_scores")


def run_cluster(n):
    import torch
    from truely_amd.gallery import FaceGallery
    gen = torch.Generator(device="cuda").manual_seed(n)
    centres = torch.nn.functional.normalize(torch.randn((n // CL_PER_ID, 512), generator=gen, device="cuda"), dim=1)
    rows = centres.repeat_interleave(CL_PER_ID, dim=0) + 0.03 * torch.randn((n, 512), generator=gen, device="cuda")
    rows = torch.nn.functional.normalize(rows, dim=1)[torch.randperm(n, generator=gen, device="cuda")]
    gal = FaceGallery(metric="cosine", capacity=n)
    gal.add(rows, range(n))
    torch.cuda.synchronize()
    for _ in range(CL_WARMUP + CL_WARM):
        info = gal.cluster(0.5, min_samples=4, return_info=True)
    torch.cuda.synchronize()
    for _ in range(CL_WARMUP + CL_WARM):
        s = gal.scores(rows)
    torch.cuda.synchronize()
    labels = info["labels"]
    print(json.dumps({"n": n, "rounds": info["rounds"], "n_clusters": info["n_clusters"], "noise": int((labels < 0).sum()),
                      "mean_degree": float(info["degree"].float().mean()), "bitmap_bytes": n * ((n + 31) // 32) * 4,
                      "score_matrix_bytes": int(s.numel()) * 4}))


def table_cluster(out):
    print("n,metric,kernel,launches_per_call,median_us_per_call,min_us_per_call,max_us_per_call,tflops,rounds,n_clusters,mean_degree,bitmap_bytes")
    for n in CL_SHAPES:
        d = os.path.join(out, f"cluster_{n}")
        info = json.load(open(os.path.join(d, "info.json")))
        tr = _trace(d)
        calls, flat = CL_WARMUP + CL_WARM, {k: [] for k in CL_KERNELS}
        for s, e, name in tr:
            for k in CL_KERNELS:
                if k in name:
                    flat[k].append(e - s)
        for k in CL_KERNELS:
            assert flat[k] and len(flat[k]) % calls == 0, (n, k, len(flat[k]))
            per = len(flat[k]) // calls
            tot = [sum(flat[k][c * per:(c + 1) * per]) / 1e3 for c in range(CL_WARMUP, calls)]
            med = statistics.median(tot)
            tf = f"{2.0 * n * n * 512 / med / 1e6:.1f}" if k in ("k_gallery_links", "k_gallery_scores") else ""
            print(f"{n},cosine,{k},{per},{med:.1f},{min(tot):.1f},{max(tot):.1f},{tf},{info['rounds']},{info['n_clusters']},"
                  f"{info['mean_degree']:.2f},{info['bitmap_bytes']}")


def run_all_cluster(out):
    for n in CL_SHAPES:
        d = os.path.join(out, f"cluster_{n}")
        os.makedirs(d, exist_ok=True)
        r = subprocess.run(["rocprofv3", "--kernel-trace", "-d", d, "-o", "t", "-f", "csv", "--", sys.executable, os.path.abspath(__file__),
                            "run-cluster", str(n)], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(f"cluster shape {n} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, file=sys.stderr, flush=True)
        open(os.path.join(d, "info.json"), "w").write(line)
    table_cluster(out)


CLL_SHAPES, CLL_PER_ID, CLL_LANES, CLL_BITMAP_MAX_N = CL_SHAPES + (131_072,), (16, 128, 1024), (4, 16, 64), 65_536
CLL_LIST_KERNELS = ("k_cluster_list_degree", "k_cluster_list_hook", "k_cluster_list_assign")
CLL_BITMAP_KERNELS = ("k_gallery_links", "k_cluster_degree", "k_cluster_hook", "k_cluster_assign")


def run_cluster_lists(n, per_id):
    import ctypes as C
    import torch
    from truely_amd import _lib
    from truely_amd.gallery import FaceGallery
    gen = torch.Generator(device="cuda").manual_seed(n)
    centres = torch.nn.functional.normalize(torch.randn((n // per_id, 512), generator=gen, device="cuda"), dim=1)
    rows = centres.repeat_interleave(per_id, dim=0) + 0.03 * torch.randn((n, 512), generator=gen, device="cuda")
    rows = torch.nn.functional.normalize(rows, dim=1)[torch.randperm(n, generator=gen, device="cuda")]
    gal = FaceGallery(metric="cosine", capacity=n)
    gal.add(rows, range(n))
    del rows, centres
    lib, ptr = gal.lib, lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    calls = CL_WARMUP + CL_WARM
    torch.cuda.synchronize()
    for _ in range(calls):
        off, idx, _sc = gal.range_search(threshold=0.5)
    del _sc
    torch.cuda.synchronize()
    out = [torch.empty((n,), dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.uint8)]
    count = torch.zeros((1,), dtype=torch.int32, device="cuda")
    need = lib.trl_cluster_lists_workspace(n)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    rounds, labels = {}, {}
    for lanes in CLL_LANES:
        r = C.c_int(0)
        for _ in range(calls):
            _lib.check(lib.trl_cluster_labels_lists(ptr(off), ptr(idx), None, n, 4, lanes, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(count),
                                                    ptr(ws), need, C.byref(r), stream))
        torch.cuda.synchronize()
        rounds[lanes], labels[lanes] = r.value, out[1].clone()
    same, bitmap_rounds = all(torch.equal(labels[4], labels[lanes]) for lanes in CLL_LANES), None
    if n <= CLL_BITMAP_MAX_N:
        for _ in range(calls):
            info = gal.cluster(0.5, min_samples=4, return_info=True, method="bitmap")
        torch.cuda.synchronize()
        same, bitmap_rounds = same and torch.equal(info["labels"], labels[4]) and torch.equal(info["degree"], out[0]), info["rounds"]
    print(json.dumps({"n": n, "per_id": per_id, "links": int(off[-1]), "mean_list": float(off[-1]) / n, "longest_list": int((off[1:] - off[:-1]).max()),
                      "rounds": rounds, "bitmap_rounds": bitmap_rounds, "n_clusters": int(count.item()), "labels_equal": bool(same),
                      "workspace_bytes": int(need)}))


def table_cluster_lists(out):
    print("n,rows_per_identity,metric,what,lanes_per_row,launches_per_call,median_us_per_call,min_us_per_call,max_us_per_call,rounds,links,"
          "mean_list,longest_list,n_clusters,labels_equal")
    calls = CL_WARMUP + CL_WARM
    for n in CLL_SHAPES:
        for per_id in CLL_PER_ID:
            d = os.path.join(out, f"cluster_lists_{n}_{per_id}")
            if not os.path.exists(os.path.join(d, "info.json")):
                continue
            info = json.load(open(os.path.join(d, "info.json")))
            tr = _trace(d)
            tail = f"{info['links']},{info['mean_list']:.2f},{info['longest_list']},{info['n_clusters']},{info['labels_equal']}"

            def row(what, lanes, times, rounds):
                assert times and len(times) % calls == 0, (n, per_id, what, lanes, len(times))
                per = len(times) // calls
                tot = [sum(times[c * per:(c + 1) * per]) / 1e3 for c in range(CL_WARMUP, calls)]
                print(f"{n},{per_id},cosine,{what},{lanes},{per},{statistics.median(tot):.1f},{min(tot):.1f},{max(tot):.1f},{rounds},{tail}")

            for k in RG_KERNELS:
                row(k, "", [e - s for s, e, name in tr if k in name], "")
            degree = [e - s for s, e, name in tr if "k_cluster_list_degree" in name]
            for i, lanes in enumerate(CLL_LANES):             # (the lanes' calls follow one another)
                row("k_cluster_list_degree", lanes, degree[i * calls:(i + 1) * calls], info["rounds"][str(lanes)])
                for k in CLL_LIST_KERNELS[1:]:
                    row(k, lanes, [e - s for s, e, name in tr if re.search(rf"{k}<(\(int\))?{lanes}>", name)], info["rounds"][str(lanes)])
            if info["bitmap_rounds"] is not None:
                for k in CLL_BITMAP_KERNELS:
                    row(k, "", [e - s for s, e, name in tr if k in name], info["bitmap_rounds"])


def run_all_cluster_lists(out):
    for n in CLL_SHAPES:
        for per_id in CLL_PER_ID:
            d = os.path.join(out, f"cluster_lists_{n}_{per_id}")
            os.makedirs(d, exist_ok=True)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "-d", d, "-o", "t", "-f", "csv", "--", sys.executable, os.path.abspath(__file__),
                                "run-cluster-lists", str(n), str(per_id)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"cluster-lists shape {n} / {per_id} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, file=sys.stderr, flush=True)
            open(os.path.join(d, "info.json"), "w").write(line)
    table_cluster_lists(out)


HI_EDGES, HI_TORCH_MAX_N = 1000, 8192


def run_hist(n):
    import torch
    from truely_amd.gallery import FaceGallery
    gen = torch.Generator(device="cuda").manual_seed(n)
    centres = torch.nn.functional.normalize(torch.randn((n // CL_PER_ID, 512), generator=gen, device="cuda"), dim=1)
    rows = centres.repeat_interleave(CL_PER_ID, dim=0) + 0.03 * torch.randn((n, 512), generator=gen, device="cuda")
    perm = torch.randperm(n, generator=gen, device="cuda")
    rows = torch.nn.functional.normalize(rows, dim=1)[perm]
    ids = perm // CL_PER_ID
    labels = ids.tolist()
    edges = torch.linspace(-1, 1, HI_EDGES)
    gal = FaceGallery(metric="cosine", capacity=n)
    gal.add(rows, labels)
    torch.cuda.synchronize()
    calls = CL_WARMUP + CL_WARM
    for _ in range(calls):
        h_all = gal.score_histogram(rows, labels, edges=edges)
        h_up = gal.score_histogram(edges=edges)
    torch.cuda.synchronize()
    for _ in range(calls):
        gal.cluster(0.5, min_samples=4)
    torch.cuda.synchronize()
    for _ in range(calls):
        gal.scores(rows)
    torch.cuda.synchronize()
    agree = None
    if n <= HI_TORCH_MAX_N:
        e_dev, slots = h_all["edges"], HI_EDGES + 2
        for _ in range(calls):
            s = gal.scores(rows)
            b = torch.bucketize(s, e_dev, right=True)             # (cosine's rule: edges <= score; these inputs give no NaN)
            b += (ids[:, None] == ids[None, :]) * slots
            c = torch.bincount(b.flatten(), minlength=2 * slots).reshape(2, slots)
        torch.cuda.synchronize()
        agree = bool(torch.equal(c[0, :-1], h_all["impostor"]) and torch.equal(c[1, :-1], h_all["genuine"]))
    diag = n                                                  # ALL = 2 UPPER + the diagonal (genuine)
    total_all = int(h_all["genuine"].sum() + h_all["impostor"].sum() + h_all["nan"].sum())
    total_up = int(h_up["genuine"].sum() + h_up["impostor"].sum() + h_up["nan"].sum())
    print(json.dumps({"n": n, "edges": HI_EDGES, "pairs_all": total_all, "pairs_upper": total_up, "all_is_2_upper_plus_diagonal":
                      total_all == 2 * total_up + diag, "torch_counts_equal": agree,
                      "occupied_bins_impostor": int((h_all["impostor"] > 0).sum()), "occupied_bins_genuine": int((h_all["genuine"] > 0).sum()),
                      "workspace_bytes": int(gal.lib.trl_gallery_hist_workspace(n, n, HI_EDGES, 0))}))


def table_hist(out):
    print("n,metric,edges,what,launches_per_call,median_us_per_call,min_us_per_call,max_us_per_call,tflops,over_links,over_hist_all,"
          "occupied_bins_impostor,workspace_bytes,torch_counts_equal")
    for n in CL_SHAPES:
        d = os.path.join(out, f"hist_{n}")
        info = json.load(open(os.path.join(d, "info.json")))
        tr = _trace(d)
        calls = CL_WARMUP + CL_WARM
        per_call = {}                                         # what -> [us per call], warm-up included

        def series(key, times, per):
            assert times and len(times) == per * calls, (n, key, len(times))
            per_call[key] = (per, [sum(times[c * per:(c + 1) * per]) / 1e3 for c in range(calls)])

        hist = [e - s for s, e, name in tr if "k_gallery_hist" in name and "k_gallery_hist_sum" not in name]
        sums = [e - s for s, e, name in tr if "k_gallery_hist_sum" in name]
        series("k_gallery_hist ALL", hist[0::2], 1)           # the calls alternate: ALL, UPPER
        series("k_gallery_hist UPPER", hist[1::2], 1)
        series("k_gallery_hist_sum ALL", sums[0::2], 1)
        series("k_gallery_links", [e - s for s, e, name in tr if "k_gallery_links" in name], 1)
        at = [i for i, r in enumerate(tr) if "k_gallery_scores" in r[2]]
        if n <= HI_TORCH_MAX_N:                               # the last `calls` k_gallery_scores launches open a torch-route call each
            assert len(at) == 2 * calls, (n, len(at))
            series("k_gallery_scores", [tr[i][1] - tr[i][0] for i in at[:calls]], 1)
            per = at[calls + 1] - at[calls]                   # kernels of one call (behind the last call come the run's own checks)
            route = [sum(e - s for s, e, _name in tr[a:a + per]) for a in at[calls:]]
            per_call["scores + bucketize + bincount"] = (per, [t / 1e3 for t in route])
        else:
            assert len(at) == calls, (n, len(at))
            series("k_gallery_scores", [tr[i][1] - tr[i][0] for i in at], 1)
        med = {k: statistics.median(v[CL_WARMUP:]) for k, (_p, v) in per_call.items()}
        for k, (per, v) in per_call.items():
            v = v[CL_WARMUP:]
            flop = {"k_gallery_hist ALL": 2.0 * n * n * 512, "k_gallery_hist UPPER": 1.0 * n * (n - 1) * 512,
                    "k_gallery_links": 2.0 * n * n * 512, "k_gallery_scores": 2.0 * n * n * 512}.get(k)
            tf = f"{flop / med[k] / 1e6:.1f}" if flop else ""
            print(f"{n},cosine,{info['edges']},{k},{per},{med[k]:.1f},{min(v):.1f},{max(v):.1f},{tf},{med[k] / med['k_gallery_links']:.3f},"
                  f"{med[k] / med['k_gallery_hist ALL']:.3f},{info['occupied_bins_impostor']},{info['workspace_bytes']},{info['torch_counts_equal']}")


def run_all_hist(out):
    for n in CL_SHAPES:
        d = os.path.join(out, f"hist_{n}")
        os.makedirs(d, exist_ok=True)
        r = subprocess.run(["rocprofv3", "--kernel-trace", "-d", d, "-o", "t", "-f", "csv", "--", sys.executable, os.path.abspath(__file__),
                            "run-hist", str(n)], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(f"hist shape {n} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, file=sys.stderr, flush=True)
        open(os.path.join(d, "info.json"), "w").write(line)
    table_hist(out)


RG_SHAPES = ((4_096, 4_096), (16_384, 16_384), (65_536, 65_536), (256, 1_000_000))
RG_THR, RG_ALL_THR, RG_DENSE_N, RG_SCORES_MAX_BYTES = 0.5, -2.0, 4_096, 2 << 30
RG_KERNELS = ("k_gallery_range_count", "k_range_rows", "k_range_scan", "k_gallery_range_fill")


def run_range(n, m):
    import torch
    from truely_amd.gallery import FaceGallery
    gen = torch.Generator(device="cuda").manual_seed(m)
    centres = torch.nn.functional.normalize(torch.randn((m // CL_PER_ID, 512), generator=gen, device="cuda"), dim=1)
    rows = centres.repeat_interleave(CL_PER_ID, dim=0) + 0.03 * torch.randn((m, 512), generator=gen, device="cuda")
    rows = torch.nn.functional.normalize(rows, dim=1)[torch.randperm(m, generator=gen, device="cuda")]
    gal = FaceGallery(metric="cosine", capacity=m)
    gal.add(rows, range(m))
    self_mode = n == m
    q = None if self_mode else rows[:n].contiguous()
    torch.cuda.synchronize()
    dense = None
    for _ in range(CL_WARMUP + CL_WARM):
        off, idx, sc = gal.range_search(q, threshold=RG_THR)
        if self_mode and n == RG_DENSE_N:
            dense = gal.range_search(q, threshold=RG_ALL_THR)
        if self_mode:
            gal.cluster(RG_THR, min_samples=4)
        if n * m * 4 <= RG_SCORES_MAX_BYTES:
            gal.scores(rows if self_mode else q)
    torch.cuda.synchronize()                                  # (not per round: a kernel that starts on a drained queue runs longer)
    same = None
    if self_mode and n <= HI_TORCH_MAX_N:
        for _ in range(CL_WARMUP + CL_WARM):
            s = gal.scores(rows)
            hit = s >= RG_THR
            hit.fill_diagonal_(False)
            rc = torch.nonzero(hit)
        torch.cuda.synchronize()
        counts = torch.bincount(rc[:, 0], minlength=n)
        same = bool(torch.equal(rc[:, 1].to(torch.int32), idx) and torch.equal(counts, off[1:] - off[:-1]) and torch.equal(s[hit], sc))
    print(json.dumps({"n": n, "m": m, "self": self_mode, "hits": int(off[-1]), "hits_dense": None if dense is None else int(dense[0][-1]),
                      "longest_row": int((off[1:] - off[:-1]).max()), "torch_lists_equal": same,
                      "workspace_bytes": int(gal.lib.trl_gallery_range_workspace(n, m, 0))}))


def table_range(out):
    print("n,m,metric,threshold,what,launches_per_call,median_us_per_call,min_us_per_call,max_us_per_call,tflops,over_links,over_scores,hits,"
          "workspace_bytes,torch_lists_equal")
    calls = CL_WARMUP + CL_WARM
    for n, m in RG_SHAPES:
        d = os.path.join(out, f"range_{n}_{m}")
        if not os.path.exists(os.path.join(d, "info.json")):
            continue
        info = json.load(open(os.path.join(d, "info.json")))
        tr = _trace(d)
        phases = [(RG_THR, info["hits"])] + ([(RG_ALL_THR, info["hits_dense"])] if info["hits_dense"] is not None else [])
        per_call = {}                                         # (threshold, what) -> (hits, [us per call], warm-up included)
        for k in RG_KERNELS:
            times = [e - s for s, e, name in tr if k in name]
            assert len(times) == len(phases) * calls, (n, m, k, len(times))
            for p, (thr, hits) in enumerate(phases):          # the phases alternate within a round
                per_call[(thr, k)] = (hits, [t / 1e3 for t in times[p::len(phases)]])
        for thr, hits in phases:
            per_call[(thr, "range_search (all four)")] = (hits, [sum(per_call[(thr, k)][1][c] for k in RG_KERNELS) for c in range(calls)])
        links = [(e - s) / 1e3 for s, e, name in tr if "k_gallery_links" in name]
        at = [i for i, r in enumerate(tr) if "k_gallery_scores" in r[2]]
        if links:
            assert len(links) == calls, (n, m, len(links))
            per_call[("", "k_gallery_links")] = ("", links)
        if info["torch_lists_equal"] is not None:             # the last `calls` k_gallery_scores launches open a torch-route call each
            assert len(at) == 2 * calls, (n, m, len(at))
            per = at[calls + 1] - at[calls]
            per_call[(RG_THR, "scores + compare + nonzero")] = (info["hits"], [sum(e - s for s, e, _n in tr[a:a + per]) / 1e3 for a in at[calls:]])
            at = at[:calls]
        if at:
            assert len(at) == calls, (n, m, len(at))
            per_call[("", "k_gallery_scores")] = ("", [(tr[i][1] - tr[i][0]) / 1e3 for i in at])
        med = {k: statistics.median(v[CL_WARMUP:]) for k, (_h, v) in per_call.items()}
        for (thr, what), (hits, v) in per_call.items():
            v = v[CL_WARMUP:]
            mk = med[(thr, what)]
            flop = 2.0 * n * m * 512 if what in ("k_gallery_range_count", "k_gallery_range_fill", "k_gallery_links", "k_gallery_scores") else None
            tf = f"{flop / mk / 1e6:.1f}" if flop else ""
            ol = f"{mk / med[('', 'k_gallery_links')]:.3f}" if ("", "k_gallery_links") in med else ""
            osc = f"{mk / med[('', 'k_gallery_scores')]:.3f}" if ("", "k_gallery_scores") in med else ""
            launches = 4 if what.startswith("range_search") else "" if what.startswith("scores +") else 1
            print(f"{n},{m},cosine,{thr},{what},{launches},{mk:.1f},{min(v):.1f},{max(v):.1f},{tf},{ol},{osc},{hits},{info['workspace_bytes']},"
                  f"{info['torch_lists_equal']}")


def run_all_range(out):
    for n, m in RG_SHAPES:
        d = os.path.join(out, f"range_{n}_{m}")
        os.makedirs(d, exist_ok=True)
        r = subprocess.run(["rocprofv3", "--kernel-trace", "-d", d, "-o", "t", "-f", "csv", "--", sys.executable, os.path.abspath(__file__),
                            "run-range", str(n), str(m)], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(f"range shape {n} x {m} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, file=sys.stderr, flush=True)
        open(os.path.join(d, "info.json"), "w").write(line)
    table_range(out)


GG_KS, GG_PER_ID = (1, 5, 16), 8
GG_WHAT = ("k_gallery_search", "k_gallery_search_groups distinct ids", "k_gallery_search_groups 8 rows per id")


def run_groups(m, n):
    import ctypes as C
    import torch
    from truely_amd import _lib
    from truely_amd.gallery import FaceGallery
    gen = torch.Generator(device="cuda").manual_seed(m + n)
    ids_n = max(m // GG_PER_ID, 1)
    centres = torch.nn.functional.normalize(torch.randn((ids_n, 512), generator=gen, device="cuda"), dim=1)
    perm = torch.randperm(m, generator=gen, device="cuda")
    ident = (perm % ids_n).to(torch.int32)                    # the identity of each enrolled row, scattered over the gallery
    rows = torch.nn.functional.normalize(centres[ident.long()] + 0.03 * torch.randn((m, 512), generator=gen, device="cuda"), dim=1)
    qid = torch.randint(0, ids_n, (n,), generator=gen, device="cuda")
    q = torch.nn.functional.normalize(centres[qid] + 0.03 * torch.randn((n, 512), generator=gen, device="cuda"), dim=1)
    del centres
    gal = FaceGallery(metric="cosine", capacity=m)
    gal.add(rows, range(m))
    del rows
    distinct = torch.arange(m, dtype=torch.int32, device="cuda")
    lib, ptr = gal.lib, lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def grouped(gid, k):
        out = (torch.empty((n, k), dtype=torch.float32, device="cuda"), torch.empty((n, k), dtype=torch.int32, device="cuda"),
               torch.empty((n, k), dtype=torch.int32, device="cuda"))
        need = lib.trl_gallery_search_groups_workspace(n, m, k, 0)
        ws = torch.empty((need,), dtype=torch.uint8, device="cuda") if need else None
        _lib.check(lib.trl_gallery_search_groups(ptr(q), None, n, ptr(gal._mat), gal.ld, ptr(gal._n2), ptr(gid), m, 0, k, ptr(out[0]), ptr(out[1]),
                                                 ptr(out[2]), ptr(ws), need, 0, stream))
        return out

    torch.cuda.synchronize()
    last = {}
    for _ in range(CL_WARMUP + CL_WARM):
        for k in GG_KS:
            last[k] = (gal.search(q, k=k), grouped(distinct, k), grouped(ident, k))
    torch.cuda.synchronize()                                  # (not per round: a kernel that starts on a drained queue runs longer)
    same, own, filled = True, 0.0, 0.0
    for k in GG_KS:
        (idx, sc), d, g = last[k]
        same = same and bool(torch.equal(idx, d[1]) and torch.equal(idx, d[2]) and torch.equal(sc.view(torch.int32), d[0].view(torch.int32)))
        live = g[2] >= 0
        per_row = [len(set(r[r >= 0].tolist())) == int((r >= 0).sum()) for r in g[2].cpu()]
        same = same and all(per_row) and bool((ident[g[1][live].long()] == g[2][live]).all())
        own, filled = float((g[2][:, 0] == qid.to(torch.int32)).float().mean()), float(live.float().mean())
    print(json.dumps({"m": m, "n": n, "identities": ids_n, "distinct_equals_search": same, "first_is_own_identity": own, "slots_filled_k16": filled,
                      "workspace_bytes_k16": int(lib.trl_gallery_search_groups_workspace(n, m, 16, 0)),
                      "search_workspace_bytes_k16": int(lib.trl_gallery_search_workspace(n, m, 16, 0))}))


def table_groups(out):
    print("m,n,k,metric,what,launches,median_us,min_us,max_us,merge_median_us,over_search,distinct_equals_search,workspace_bytes_k16")
    calls = CL_WARMUP + CL_WARM
    for m in M_SHAPES:
        for n in N_SHAPES:
            d = os.path.join(out, f"groups_{m}_{n}")
            if not os.path.exists(os.path.join(d, "info.json")):
                continue
            info = json.load(open(os.path.join(d, "info.json")))
            launches = []                                     # per call, in launch order: [main ns, merge ns]
            for s, e, name in _trace(d):
                if "k_gallery_merge" in name:
                    launches[-1][1] = e - s
                elif "k_gallery_search" in name:
                    launches.append([e - s, 0, "k_gallery_search_groups" in name])
            assert len(launches) == calls * len(GG_KS) * 3, (m, n, len(launches))
            for ki, k in enumerate(GG_KS):
                med = {}
                for w, what in enumerate(GG_WHAT):
                    part = [launches[(r * len(GG_KS) + ki) * 3 + w] for r in range(CL_WARMUP, calls)]
                    assert all(p[2] == (w > 0) for p in part), (m, n, k, what)
                    tot = [(a + b) / 1e3 for a, b, _g in part]
                    med[what] = statistics.median(tot)
                    print(f"{m},{n},{k},cosine,{what},{len(part)},{med[what]:.1f},{min(tot):.1f},{max(tot):.1f},"
                          f"{statistics.median(b for _a, b, _g in part) / 1e3:.1f},{med[what] / med[GG_WHAT[0]]:.3f},{info['distinct_equals_search']},"
                          f"{info['workspace_bytes_k16'] if w else info['search_workspace_bytes_k16']}")


def run_all_groups(out):
    for m in M_SHAPES:
        for n in N_SHAPES:
            d = os.path.join(out, f"groups_{m}_{n}")
            os.makedirs(d, exist_ok=True)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "-d", d, "-o", "t", "-f", "csv", "--", sys.executable, os.path.abspath(__file__),
                                "run-groups", str(m), str(n)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"groups shape {m} x {n} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, file=sys.stderr, flush=True)
            open(os.path.join(d, "info.json"), "w").write(line)
    table_groups(out)


def run_all(out):
    for m in M_SHAPES:
        for n in N_SHAPES:
            d = os.path.join(out, f"{m}_{n}")
            os.makedirs(d, exist_ok=True)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "-d", d, "-o", "t", "-f", "csv", "--", sys.executable, os.path.abspath(__file__),
                                "run", str(m), str(n)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"shape {m} x {n} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, file=sys.stderr, flush=True)
            open(os.path.join(d, "info.json"), "w").write(line)
    table(out)


if __name__ == "__main__":
    if sys.argv[1] == "--all":
        run_all(sys.argv[2])
    elif sys.argv[1] == "--table":
        table(sys.argv[2])
    elif sys.argv[1] == "--cluster":
        run_all_cluster(sys.argv[2])
    elif sys.argv[1] == "--cluster-table":
        table_cluster(sys.argv[2])
    elif sys.argv[1] == "run-cluster":
        run_cluster(int(sys.argv[2]))
    elif sys.argv[1] == "--cluster-lists":
        run_all_cluster_lists(sys.argv[2])
    elif sys.argv[1] == "--cluster-lists-table":
        table_cluster_lists(sys.argv[2])
    elif sys.argv[1] == "run-cluster-lists":
        run_cluster_lists(int(sys.argv[2]), int(sys.argv[3]))
    elif sys.argv[1] == "--hist":
        run_all_hist(sys.argv[2])
    elif sys.argv[1] == "--hist-table":
        table_hist(sys.argv[2])
    elif sys.argv[1] == "run-hist":
        run_hist(int(sys.argv[2]))
    elif sys.argv[1] == "--range":
        run_all_range(sys.argv[2])
    elif sys.argv[1] == "--range-table":
        table_range(sys.argv[2])
    elif sys.argv[1] == "run-range":
        run_range(int(sys.argv[2]), int(sys.argv[3]))
    elif sys.argv[1] == "--groups":
        run_all_groups(sys.argv[2])
    elif sys.argv[1] == "--groups-table":
        table_groups(sys.argv[2])
    elif sys.argv[1] == "run-groups":
        run_groups(int(sys.argv[2]), int(sys.argv[3]))
    else:
        run(int(sys.argv[2]), int(sys.argv[3]))
