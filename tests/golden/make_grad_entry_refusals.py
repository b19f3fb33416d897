"""Writes tests/golden/grad_entry_refusals.npz: the table of
tests/test_grad_entry_refusals_host.py::grad_entry_refusal_table -- `rows` (entry, base, first and second deviation, return
code, message index, workspace bytes) and `messages`, the distinct texts of rk_last_error() with the registration id replaced by
a fixed token.  The archive carries a fixed date, so that the same table gives the same bytes.
Needs a built library, no GPU.  Run from the repository root."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from test_grad_entry_refusals_host import GOLDEN, write_table

rows, messages = write_table(GOLDEN)
print("written", rows.shape, len(messages), "distinct messages, return codes", dict(zip(*np.unique(rows[:, 4], return_counts=True))))
