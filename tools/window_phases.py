"""Per-step latency of k_window_f (diagnostic build, SMX_LIB=<-DSMX_DIAG=1 build>: the
k_window_f<CAP, NT, true, false> instances, the shipped order with stamps): lane 0 of each
workgroup stamps s_memtime at its start and after every step (smx_window.h, WSTAMP); this
prints the mean cycles of each step per window, and the window-kernel time with and without
stamping.  usage: window_phases.py [n_ops] [config]"""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
NST = 16  # WF_NSTAMP
# stamp i is taken after step i of smx_window.h (0: the window's start)
NAMES = ["start", "load", "heads", "run-index", "group-count", "group-scan", "buckets", "bucket-scan",
         "members", "rank", "renrank", "stage1+posl", "flags+cand", "write1", "stage2+write2"]
LAST = len(NAMES) - 1


def main():
    import torch
    from semantic_merge_amd import _lib, synth
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    cfg = sys.argv[2] if len(sys.argv) > 2 else "c3"
    spec = synth.LiftSpec(**{**synth.CONFIGS[cfg].__dict__, "n_total": n})
    soa = synth.lift_soa(synth.lift_logs(spec))
    dc = _lib.DeviceCompose(soa)
    lib = _lib.lib()
    W = n // 256 + 16
    buf = torch.zeros(W * NST, dtype=torch.int64, device="cuda")

    def timed(reps=5):  # the normal and the wide windows' stage (a log runs one of them to the end)
        lib.smx_reset_stage_times()
        lib.smx_set_profiling(1)
        for _ in range(reps):
            dc.run()
        torch.cuda.synchronize()
        lib.smx_set_profiling(0)
        st = _lib.stage_times()
        return (st["window"][0] + st["window_wide"][0]) / reps

    dc.run()
    print(f"window plain   {timed():.3f} ms  (median of 3: {sorted(timed() for _ in range(3))[1]:.3f})")
    try:
        lib.smx_debug_phase_buffer
    except AttributeError:
        return
    lib.smx_debug_phase_buffer(ctypes.c_void_p(buf.data_ptr()), ctypes.c_size_t(buf.numel() * 8))
    dc.run()
    print(f"window stamped {timed():.3f} ms")
    buf.zero_()
    dc.run()
    torch.cuda.synchronize()
    lib.smx_debug_phase_buffer(None, ctypes.c_size_t(0))
    a = buf.cpu().numpy().reshape(-1, NST)
    a = a[a[:, LAST] != 0][:, :LAST + 1]  # (a window of a failed plan leaves before its last stamp)
    print(f"{len(a)} windows stamped")
    ok = (a != 0).all(axis=1) & (np.diff(a, axis=1) >= 0).all(axis=1)
    print(f"stamps non-zero and non-decreasing in step order: {int(ok.sum())} of {len(a)} windows")
    tot = (a[:, LAST] - a[:, 0]).mean()
    for i in range(1, LAST + 1):
        d = (a[:, i] - a[:, i - 1]).mean()
        print(f"  {i:2d} {NAMES[i]:13s} {d:9.0f} cyc  {100 * d / tot:5.1f}%")
    print(f"  {'total':16s} {tot:9.0f} cyc per window (lane-0 view)")
    st = np.sort(a[:, 0])
    print(f"  window start span {(st[-1] - st[0]):.0f} cyc; concurrent ~ {tot * len(a) / (a[:, LAST].max() - st[0]):.0f} windows")


if __name__ == "__main__":
    main()
