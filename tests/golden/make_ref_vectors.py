"""Writes tests/golden/ref_vectors.npz: what the reference's own helpers return for the fixed inputs of tests/ref_vectors.py, computed
with the libraries oracle/Makefile compiles from the reference tree into oracle/_ref (build() does that where the tree is present).
Re-run after changing an input there:  python tests/golden/make_ref_vectors.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ref_vectors  # noqa: E402


def main():
    ref, mazes = ref_vectors.util_lib(), ref_vectors.mazes_lib()
    if ref is None or mazes is None:
        raise SystemExit("oracle/_ref is not built: run build() where the reference tree is present")
    out = ref_vectors.util_vectors(ref)
    out.update(ref_vectors.maze_vectors(mazes))
    np.savez_compressed(ref_vectors.PATH, **out)
    print(f"wrote {ref_vectors.PATH}: {len(out)} arrays")


if __name__ == "__main__":
    main()
