#!/bin/bash
# Window step exits (SMX_ABLATE 16 = load only, 100 + N = leave after step N of
# smx_window.h, 0 = the whole kernel; diagnostic build tools/_build/var_diag) on config 5's
# shape (wide windows first, SMX_FIRST_WIDE) and on config 3's, 20M ops each, SQ counters
# per exit (tools/sq_ablate.sh):
#   bash tools/ablate_runs.sh OUTDIR      (profiles/r05_ablate, with the numbering of its time)
set -o pipefail
O=$1; mkdir -p "$O"
V="16 102 103 104 105 106 107 108 109 110 111 112 113 0"
COMPOSE_CFG=c5 SMX_FIRST_WIDE=1 bash tools/sq_ablate.sh "$O/c5" tools/_build/var_diag/libsmx.so "$V" > "$O/c5.txt" 2>&1 || { tail -5 "$O/c5.txt"; exit 1; }
bash tools/sq_ablate.sh "$O/c3" tools/_build/var_diag/libsmx.so "110 111 112 113 0" > "$O/c3.txt" 2>&1 || { tail -5 "$O/c3.txt"; exit 1; }
for f in "$O"/c5/a*.txt "$O"/c3/a*.txt; do echo "$f $(awk '/^k_window_f/{p=1} p && /dur_us/{print $2; exit}' $f)"; done
