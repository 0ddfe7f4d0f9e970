"""hamming_topk_fp4rows (tod_amd/csrc/match_fp4rows.h): the matrix-core search reading the rows from their resident fp4 copy, against the
vector-ALU engine in the same process, bit for bit (tests/fp4_rows_child.py). The knobs are read once per process, hence children:
TODHIP_K4X_FP4_ROWS=1 sends every launch of >= 4 query blocks per wave through the copy, TODHIP_K4X_QT picks 4 or 6 blocks.
Shapes: 4096, 4113 and 8191 rows in 3 objects (whole steps, a 17-row last step, a 31-row one; several tiles), 129 and 200 queries (a
padded last query block, two query waves at 4 blocks), k 1, 2, 5, radius 35, 64, 96, 255 (the lowest block form the thresholds allow:
split after 2, after 3, whole with the integer maximum, whole with the float maximum), each block form forced through
todhip_set_matcher_block_split; independent bits, rows that equal a query on their first 128 / 192 positions (the blocks go on to
their second part), duplicate rows (ties). Then the copy must follow the rows: a second load, a selection on and off, the bit order on
and off."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.gpu
@pytest.mark.parametrize("qt", [4, 6])
def test_fp4_rows_pass_equals_the_vector_engine(qt):
    env = dict(os.environ, TODHIP_K4X_FP4_ROWS="1", TODHIP_K4X_QT=str(qt))
    p = subprocess.run([sys.executable, os.path.join(HERE, "fp4_rows_child.py")], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-2000:] + p.stderr[-4000:]
    assert int(p.stdout.split()[1]) == 24 * 36 + 6 + 18 + 12 + 8
