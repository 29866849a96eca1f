"""Writes tests/golden/disk_shade_pin.json: the SHA-256 of every output array of
the CPU path's disk renders, per case of tests/test_disk_shade_pin_cpu.py.

    python tests/golden/make_disk_shade_pin.py

The committed fixture was written once, on a build of commit 284f746, and is
what a change to the shading paths of csrc/geo_disk.h is held to.  Run it again
only when the disk's f32 specification is meant to change."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import test_disk_shade_pin_cpu as P  # noqa: E402


def main():
    lib = P.AR.load_cpu()
    out = {i: P.digests(lib, *c) for i, c in zip(P.IDS, P.CASES)}
    with open(P.FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    ok = sum(v["rc"] == P.GEO_OK for v in out.values())
    print(f"{len(out)} cases, {ok} GEO_OK; {os.path.getsize(P.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
