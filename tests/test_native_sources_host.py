"""The build's file lists: every source exists, the dependency list that decides whether librva.so is stale holds every header,
and every project header a source includes is in that list.  No GPU."""
import re

from realtime_video_analytics_32streams_amd import _native as N


def test_sources_exist_and_name_the_detector_files():
    assert len(set(N.SOURCES)) == len(N.SOURCES)
    for s in N.SOURCES:
        assert (N.CSRC / s).is_file(), f"{s} is listed in SOURCES and does not exist"
    for s in ("rva_conv.hip", "rva_stem.hip", "rva_yolo_ops.hip"):
        assert s in N.SOURCES
    assert sorted(p.name for p in N.CSRC.glob("*.hip")) == sorted(N.SOURCES), "a .hip file in csrc/ that the build does not compile"


def test_build_deps_hold_every_source_and_header():
    deps = set(N.build_deps())
    assert all(d.is_file() for d in deps)
    headers = set(N.CSRC.glob("*.h"))
    assert headers and N.CSRC / "rva_conv_dev.h" in headers
    assert headers <= deps and {N.CSRC / s for s in N.SOURCES} <= deps and N.ROOT / "include" / "rva.h" in deps


def test_every_included_project_header_is_a_build_dep():
    deps = {d.name for d in N.build_deps()}
    for f in list(N.CSRC.glob("*.hip")) + list(N.CSRC.glob("*.h")):
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read_text(), flags=re.M):
            assert inc.split("/")[-1] in deps, f'{f.name} includes "{inc}", which the build does not watch'
