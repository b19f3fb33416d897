"""Writes tests/golden/grid_entry_refusals.npz: the table of
tests/test_grid_entry_refusals_host.py::grid_entry_refusal_table -- `rows` (entry, base, first and second deviation, return
code, message index) and `messages`, the distinct texts of rk_last_error() with registration ids replaced by fixed tokens.
The archive carries a fixed date, so that the same table gives the same bytes.
Needs a built library, no GPU.  Run from the repository root."""
import io, os, sys, zipfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.test_grid_entry_refusals_host import GOLDEN, grid_entry_refusal_table

rows, messages = grid_entry_refusal_table()
with zipfile.ZipFile(GOLDEN, "w") as z:
    for name, array in (("rows", rows), ("messages", messages)):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, array, allow_pickle=False)
        info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        z.writestr(info, buf.getvalue())
print("written", rows.shape, len(messages), "distinct messages, return codes", dict(zip(*np.unique(rows[:, 4], return_counts=True))))
