# the matrix-core matcher's DB pass alone at 32 000 x 1M (tools/k4x_one.py), per block form (split after 2, after 3, whole), reading the
# packed rows (TODHIP_K4X_FP4_ROWS=0) against their resident fp4 copy (=1), alternating; then by launch size, 1 to 16 frames of 1000
# queries, adaptive block form (profiles/match_fp4_rows.json)
cd "$(dirname "$0")/.."
for half in 2 3 0; do
  for fp4 in 0 1 0 1; do
    echo -n "split $half copy $fp4: "; B=32 TODHIP_K4X_HALF=$half TODHIP_K4X_FP4_ROWS=$fp4 timeout -k 10 200 python tools/k4x_one.py mfma 2>&1 | tail -1
  done
done
for B in 1 2 3 4 8 16; do
  for fp4 in 0 1 0 1; do
    echo -n "frames $B copy $fp4: "; B=$B TODHIP_K4X_FP4_ROWS=$fp4 timeout -k 10 200 python tools/k4x_one.py mfma 2>&1 | tail -1
  done
done
