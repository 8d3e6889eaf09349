"""What the crafted encoder images of tests/jpeg_enc_craft.py exercise in K7's entropy coder -> profiles/jpeg_enc_craft.json.

No GPU: the figures come from ``oracle/jpeg_oracle.py`` through ``jpeg_enc_craft.facts``.  Per image its geometry, intervals, passes
per interval and largest coded block; over the set the (run, size) symbols coded per AC table (of 160), the ZRL chain lengths, the
blocks without EOB and of EOB only, the DC categories per component (signed), the pinned noise image that shows each stuffing
fact of the kernel's 64-byte steps and 64-block passes, and the largest single block in bits beside the 1728 bits of K7's private
buffer.  tests/test_jpeg_enc_craft_host.py requires the committed file to equal what this prints.
Usage: python tools/jpeg_enc_craft_report.py [--out profiles/jpeg_enc_craft.json]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tests import jpeg_enc_craft as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rep = E.coverage()
    text = json.dumps(rep, indent=1) + "\n"
    if args.out:
        Path(args.out).write_text(text)
    print(json.dumps({k: v for k, v in rep.items() if k != "images"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
