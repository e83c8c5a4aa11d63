"""Writes tests/golden/functional_descs.json: what src/ops/functional.py hands the library -- entry point, descriptor fields, plain
numbers -- and what it returns, for every shape question and every descriptor-building launch wrapper over the lists of
tests/_functional_replay.py, recorded through that module's stand-in library on CPU tensors (no GPU, no built library).

Run it on the commit whose behaviour is to be pinned, BEFORE changing how functional.py asks or builds:
    python tools/gen_golden_functional.py
tests/test_functional_queries_cpu.py replays the same lists and compares entry for entry."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "image-generation-models_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

if __name__ == "__main__":
    import _functional_replay as R
    from src.ops import functional as K
    rec = R.replay(K)
    path = os.path.join(ROOT, "tests", "golden", "functional_descs.json")
    with open(path, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(rec['questions'])} questions, {len(rec['wrappers'])} wrapper cases, {os.path.getsize(path)} bytes")
