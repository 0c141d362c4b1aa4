"""Who releases device memory, pinned memory, streams and events in tools_amd/csrc: the four owners of psf_hip_util.hpp and nobody else.

A handle's or a call's resource is a DevArr / PinArr / Stream / Event member or local and dies with its owner, so no source file has a release list to keep
in step.  A new call of one of the four release functions anywhere else fails here until it is entered in ALLOWED, by file and function."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools_amd", "csrc")
RELEASES = ("hipFree", "hipHostFree", "hipStreamDestroy", "hipEventDestroy")

# (file, function) -> release calls allowed there.  Empty today: the resources that live as long as the process are never released at all --
# the per-device events of WalkTurn (psfgpv_impl.hpp), the plan cache's d_zetas (psf_ntt.hip) -- and the signals of psf_sdma.hpp are HSA's, dropped by
# HostPipe::~HostPipe through SdmaCopy::drop_signal.
ALLOWED = {}


def _code(text):
    """The text without // and /* */ comments (no string literal of these sources holds a comment marker or a release name)."""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _enclosing_function(code, pos):
    """Name of the last function-like definition that opens at column 0 before `pos` (the sources define every function at column 0)."""
    best = None
    for m in re.finditer(r"^(?:[A-Za-z_][\w:<>,\*&\s]*?)\b([A-Za-z_~][\w:~]*)\s*\([^;{}]*\)\s*(?:const\s*)?(?:noexcept\s*)?\{", code[:pos], flags=re.M):
        best = m.group(1)
    return best


def _sites():
    out = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp", ".cpp", ".h")):
            continue
        code = _code(open(os.path.join(CSRC, name)).read())
        for m in re.finditer(r"\b(%s)\b" % "|".join(RELEASES), code):
            out.append((name, _enclosing_function(code, m.start()), m.group(1), code.count("\n", 0, m.start()) + 1))
    return out


def test_release_calls_only_in_the_owners():
    sites = _sites()
    stray = [s for s in sites if s[0] != "psf_hip_util.hpp" and s[2] not in ALLOWED.get((s[0], s[1]), ())]
    assert not stray, "release calls outside psf_hip_util.hpp (file, function, call, line): %r" % stray
    # inside psf_hip_util.hpp each release function is named once: as the release of its owner
    inside = sorted(s[2] for s in sites if s[0] == "psf_hip_util.hpp")
    assert inside == sorted(RELEASES), inside
    text = _code(open(os.path.join(CSRC, "psf_hip_util.hpp")).read())
    for alias, call in (("DevArr", "hipFree"), ("PinArr", "hipHostFree"), ("Stream", "hipStreamDestroy"), ("Event", "hipEventDestroy")):
        assert re.search(r"using %s = Owned(?:Arr)?<[^;]*\b%s>;" % (alias, call), text), (alias, call)


def test_the_scan_sees_a_release_call():
    """The scan itself: a call in code is found with its function, one in a comment is not."""
    code = _code("static void f(int* p) {\n  // hipFree(p) in a comment\n  hipFree(p);\n}\n")
    hits = [(m.group(1), _enclosing_function(code, m.start())) for m in re.finditer(r"\b(hipFree)\b", code)]
    assert hits == [("hipFree", "f")]
