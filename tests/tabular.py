"""Order-insensitive exact comparison of operator outputs with numpy (the
python-tuple multiset in galaxysql_amd.chunk is too slow for 10^5-row
results)."""
import numpy as np

from galaxysql_amd.chunk import F64


def sorted_table(chunks, n_cols):
    """Result chunks -> (rows, 2 * n_cols) int64 matrix, rows sorted.

    Column c becomes two columns: its null flags and its value bits (f64
    viewed as int64 so == is bit-exact; values under a NULL forced to 0)."""
    if not chunks:
        return np.zeros((0, 2 * n_cols), dtype=np.int64)
    cols = []
    for c in range(n_cols):
        vals, nulls = [], []
        for ch in chunks:
            b = ch.blocks[c]
            v = np.asarray(b.values)
            v = (v.astype(np.float64).view(np.int64) if b.type == F64
                 else v.astype(np.int64))
            nl = (np.zeros(len(v), dtype=np.int64) if b.nulls is None
                  else np.asarray(b.nulls).astype(np.int64))
            vals.append(np.where(nl != 0, 0, v))
            nulls.append(nl)
        cols.append(np.concatenate(nulls))
        cols.append(np.concatenate(vals))
    m = np.stack(cols, axis=1)
    return m[np.lexsort(m.T[::-1])]
