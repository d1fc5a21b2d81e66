"""build.needs_build() watches the same headers as the compile step: every csrc/*.h and include/ldn_hip.h.
Empty files in a temporary tree, explicit mtimes; no compiler, no GPU."""
import os

from laudnet_amd import build


def _touch(path, t):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "w").close()
    os.utime(path, (t, t))


def test_needs_build_sees_every_internal_header(tmp_path, monkeypatch):
    csrc, lib, pub = tmp_path / "csrc", tmp_path / "libldn_hip.so", tmp_path / "include" / "ldn_hip.h"
    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "LIB", str(lib))
    monkeypatch.setattr(build, "PUBLIC_HEADER", str(pub))
    headers = ["ldn_common.h", "ldn_prims.h", "ldn_mlp.h", "ldn_chain_ld.h"]
    for name in build.SOURCES + headers:
        _touch(str(csrc / name), 1000)
    _touch(str(pub), 1000)
    assert build.needs_build(), "no library yet"
    _touch(str(lib), 2000)
    assert not build.needs_build(), "the library is newer than every source and header"
    for name in headers[1:]:                      # the case a hand-kept list of headers got wrong: a header that is not ldn_common.h
        os.utime(str(csrc / name), (3000, 3000))
        assert build.needs_build(), f"{name} is newer than the library"
        os.utime(str(csrc / name), (1000, 1000))
    os.utime(str(pub), (3000, 3000))
    assert build.needs_build(), "include/ldn_hip.h is newer than the library"
    os.utime(str(pub), (1000, 1000))
    os.utime(str(csrc / build.SOURCES[0]), (3000, 3000))
    assert build.needs_build(), "a source is newer than the library"
