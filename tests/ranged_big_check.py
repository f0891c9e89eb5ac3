"""Helper of tests/test_gpu_ranged_big.py: runs in a FRESH process (torch must initialise HIP before libsweepga_gpu.so is
loaded).  n = 2^31 + 2^26 records of the S-pan shape (100 genomes, 9,900 genome pairs) generated on the device, pair-major and
shuffled, the sweep flags and the CLI defaults: swg_filter_device (device columns) against swg_filter (host columns), the
global chain numbering over all records, and 8 sampled genome pairs against the oracle run on each pair alone.  Prints one
JSON object."""
import ctypes as C
import json
import sys
import threading
import time

import numpy as np

N = 2**31 + 2**26
G = 100
STEP = 2**30   # torch's sorts, scans and index kernels stop at 2^31 elements: every pass over the records goes in chunks


def spans(n):
    return [(a, min(a + STEP, n)) for a in range(0, n, STEP)]


def main():
    import torch
    assert torch.cuda.is_available()
    import bench
    import sweepga_amd as sw
    from sweepga_amd import _lib
    from tests import orc
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = sw.Context(0)
    lib = ctx.lib
    names = bench.span_names(G)
    out = {"n": N, "cases": {}}
    t_all = time.perf_counter()
    cols, _ = bench.gen_shard(torch, N, G, 4242, dev)
    rng = np.random.default_rng(5)
    for order in ("pair_major", "shuffled"):
        ctx.set_memory_limit(1)   # (the context's blocks back to the device for torch's passes below)
        ctx.set_memory_limit(0)
        torch.cuda.empty_cache()
        if order == "shuffled":
            # record i takes record (A * i + B) mod N: a bijection (A is a prime that does not divide N) that scatters every pair
            A, B = 1_000_003, 12_345
            for k in bench.REC_COLS:
                src, dst = cols[k], torch.empty_like(cols[k])
                for a, b in spans(N):
                    dst[a:b] = src[(torch.arange(a, b, device=dev, dtype=torch.int64) * A + B) % N]
                cols[k] = dst
                del src
            torch.cuda.synchronize()
        host = {k: cols[k].cpu().numpy() for k in bench.REC_COLS}
        pair = (cols["q_id"].to(torch.int64) * G + cols["t_id"].to(torch.int64))
        P = G * G
        first = torch.full((P,), 2**40, dtype=torch.int64, device=dev)   # first record of every pair
        for a, b in spans(N):
            first.scatter_reduce_(0, pair[a:b], torch.arange(a, b, device=dev, dtype=torch.int64), "amin")
        present = torch.nonzero(first < 2**40).flatten().cpu().numpy()
        sample = rng.choice(present, 8, replace=False)
        members = {}
        for p in sample:
            members[int(p)] = torch.cat([torch.nonzero(pair[a:b] == int(p)).flatten() + a for a, b in spans(N)]).cpu().numpy()
        for pipeline in ("sweep", "default"):
            res = {}
            cfg = bench.make_config(sw, pipeline)
            cc = cfg.to_c()
            # device columns
            status = torch.zeros(N, dtype=torch.uint8, device=dev)
            chain = torch.zeros(N, dtype=torch.int32, device=dev)
            r = bench.make_records(_lib, cols, N, G)
            stats = _lib.SwgStats()
            t0 = time.perf_counter()
            ctx.check(lib.swg_filter_device(ctx.handle, C.byref(r), C.byref(cc), C.c_void_p(status.data_ptr()),
                                            C.c_void_p(chain.data_ptr()), C.byref(stats)))
            ctx.synchronize()
            res["device_s"] = time.perf_counter() - t0
            # once more with every launch timed: the ranged path's own kernels, reported by name (ms, launches)
            ctx.profile_reset()
            ctx.profile(True)
            ctx.check(lib.swg_filter_device(ctx.handle, C.byref(r), C.byref(cc), C.c_void_p(status.data_ptr()),
                                            C.c_void_p(chain.data_ptr()), None))
            ctx.synchronize()
            ctx.profile(False)
            res["range_kernels"] = {k: [v[0], round(v[1], 2)] for k, v in ctx.profile_table().items() if k.startswith("range_")}
            res["n_out"] = int(stats.n_out)
            # the context's blocks go back to the device (a limit below them releases them) for the checks below
            ctx.set_memory_limit(1)
            ctx.set_memory_limit(0)
            # global numbering on the device: per pair, kept chains contiguous, from 1, no gaps, in order of first retained
            # record (every record of these flag sets passes the step-1 predicate: its pair's first record)
            lo = torch.full((P,), 2**40, dtype=torch.int64, device=dev)
            hi = torch.zeros(P, dtype=torch.int64, device=dev)
            top = 0
            for a, b in spans(N):
                c = chain[a:b].to(torch.int64) & 0xffffffff
                k = c != 0
                lo.scatter_reduce_(0, pair[a:b][k], c[k], "amin")
                hi.scatter_reduce_(0, pair[a:b][k], c[k], "amax")
                top = max(top, int(c.max()))
            if top:
                w = torch.nonzero(hi > 0).flatten()
                by_first = w[torch.argsort(first[w])]
                l, h = lo[by_first], hi[by_first]
                seen = torch.zeros(top + 1, dtype=torch.bool, device=dev)
                for a, b in spans(N):
                    c = chain[a:b].to(torch.int64) & 0xffffffff
                    seen[c[c != 0]] = True
                res["numbering_ok"] = bool(int(l[0]) == 1 and bool((l[1:] == h[:-1] + 1).all()) and int(h[-1]) == top
                                           and bool(seen[1:].all()))
                res["kept_chains"] = top
            else:
                res["numbering_ok"] = pipeline == "sweep"
            del lo, hi
            st_d, ch_d = status.cpu().numpy(), chain.cpu().numpy().view(np.uint32)
            del status, chain
            torch.cuda.empty_cache()
            # host columns
            hr = _lib.SwgRecords()
            hr.n = N
            for k in bench.REC_COLS:
                setattr(hr, k, host[k].ctypes.data)
            hr.n_seq = G
            gl = cols["seq_genome_last"].cpu().numpy()
            g2 = cols["seq_genome_two"].cpu().numpy()
            hr.seq_genome_last, hr.n_genome_last, hr.seq_genome_two, hr.n_genome_two = gl.ctypes.data, G, g2.ctypes.data, G
            st_h = np.empty(N, np.uint8)
            ch_h = np.empty(N, np.uint32)
            t0 = time.perf_counter()
            ctx.check(lib.swg_filter(ctx.handle, C.byref(hr), C.byref(cc), st_h.ctypes.data, ch_h.ctypes.data, C.byref(stats)))
            res["host_s"] = time.perf_counter() - t0
            res["device_equals_host"] = bool(np.array_equal(st_d, st_h) and np.array_equal(ch_d, ch_h))
            del st_h, ch_h
            # sampled pairs against the oracle on that pair alone: status exact, chain numbers up to one shift
            bad, threads = [], []
            ocfg = bench._oracle_config(cfg)
            for p in sample:
                idx = members[int(p)]
                u = lambda a: np.ascontiguousarray(a[idx].astype(np.uint64))  # noqa: E731
                rec = orc.Records([names[i] for i in host["q_id"][idx]], [names[i] for i in host["t_id"][idx]],
                                  u(host["q_start"]), u(host["q_end"]), u(host["t_start"]), u(host["t_end"]), u(host["block_len"]),
                                  np.ascontiguousarray(host["identity"][idx]), u(host["matches"]),
                                  np.where(host["strand"][idx] == 0, ord("+"), ord("-")).astype(np.uint8),
                                  np.arange(len(idx), dtype=np.uint64))

                def work(rec=rec, idx=idx, p=p):
                    ost, och = orc.apply_filters(ocfg, rec)
                    s, c = st_d[idx], ch_d[idx].astype(np.int64)
                    ok = np.array_equal(s, ost) and np.array_equal(c != 0, och != 0)
                    if ok and (c != 0).any():
                        d = c[c != 0] - och[och != 0].astype(np.int64)
                        ok = bool((d == d[0]).all())
                    if not ok:
                        bad.append(int(p))
                th = threading.Thread(target=work)
                th.start()
                threads.append(th)
            for th in threads:
                th.join()
            res["sampled_pairs"] = [int(p) for p in sample]
            res["sampled_records"] = int(sum(len(members[int(p)]) for p in sample))
            res["sampled_bad"] = bad
            out["cases"][f"{order}/{pipeline}"] = res
            del st_d, ch_d
            print(json.dumps({order + "/" + pipeline: res}), file=sys.stderr, flush=True)
        del host, pair, first
    out["wall_s"] = time.perf_counter() - t_all
    print(json.dumps(out))


if __name__ == "__main__":
    main()
