"""Generate tests/golden/reference_files_sha256.json: SHA-256 digests of the reference's test data files that
tests/files/ holds copies of (read from tests/files of the reference tree, REF of oracle/Makefile).

Run in the build container only:   python tests/golden/make_reference_files_sha256.py
"""
import hashlib
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
with open(os.path.join(ROOT, "oracle", "Makefile")) as _f:
    REF = next(ln.split("?=", 1)[1].strip() for ln in _f if ln.startswith("REF ?="))
REF_FILES = os.path.join(REF, "tests", "files")


def main():
    names = sorted(os.listdir(os.path.join(os.path.dirname(HERE), "files")))
    out = {}
    for f in names:
        with open(os.path.join(REF_FILES, f), "rb") as fh:
            out[f] = hashlib.sha256(fh.read()).hexdigest()
    with open(os.path.join(HERE, "reference_files_sha256.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
