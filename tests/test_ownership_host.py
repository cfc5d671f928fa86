"""Who may release GPU resources in libcss_mi355.so (csrc/api_ctx.hpp: DevBuf, PinnedBuf, Event), checked on the sources, no GPU:
device memory, page-locked memory and events are members of move-only owners and free themselves, so the release calls -- and
the allocations the owners pair them with -- appear nowhere else.  A buffer added as a member cannot leak; one released by hand
somewhere would be a second owner, and this test names the file."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
CALLS = ("hipFree", "hipHostFree", "hipEventDestroy", "hipMalloc", "hipHostMalloc")


def _code(path):
    """the file without comments and with its string and character literals emptied: an error text may name a call
    (css_create's "hipMalloc(weights) failed" is part of what the ABI returns), only code can make one"""
    text, out, i = open(path).read(), [], 0
    while i < len(text):
        two = text[i:i + 2]
        if two == "//":
            i = text.find("\n", i) if "\n" in text[i:] else len(text)
        elif two == "/*":
            i = text.index("*/", i) + 2
        elif text[i] in "\"'":
            q, i = text[i], i + 1
            while text[i] != q:
                i += 2 if text[i] == "\\" else 1
            i += 1
            out.append(q + q)
        else:
            out.append(text[i])
            i += 1
    return "".join(out)


def _count(text, call):
    return len(re.findall(rf"\b{call}\s*\(", text))


def _body(text, head):
    """the brace-matched body that follows the first match of `head`"""
    m = re.search(head, text)
    assert m, f"{head!r} not found"
    i = text.index("{", m.end() - 1)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i:j + 1]
        j += 1


def test_release_calls_live_only_in_the_owners():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    assert len(files) >= 20
    code = {os.path.basename(f): _code(f) for f in files}
    found = {c: {f: _count(t, c) for f, t in code.items() if _count(t, c)} for c in CALLS}
    ctx, core = code["api_ctx.hpp"], code["api_core.hip"]
    owner = {name: _body(ctx, rf"\bstruct {name}\s*\{{") for name in ("DevBuf", "PinnedBuf", "Event")}
    fn = {name: _body(core, rf"\b{name}\s*\([^;{{]*\)\s*\{{") for name in ("ensure", "dev_alloc", "css_host_alloc", "css_host_free")}

    # per file: nothing outside the header of the owners and the unit that holds ensure / css_host_*
    assert found["hipFree"] == {"api_ctx.hpp": 1}
    assert found["hipEventDestroy"] == {"api_ctx.hpp": 1}
    assert found["hipHostFree"] == {"api_ctx.hpp": 1, "api_core.hip": 1}
    assert found["hipHostMalloc"] == {"api_ctx.hpp": 1, "api_core.hip": 1}
    assert found["hipMalloc"] == {"api_core.hip": 2}
    # ... and inside those two files, only the owner or the function that is meant
    assert _count(owner["DevBuf"], "hipFree") == 1
    assert _count(owner["Event"], "hipEventDestroy") == 1
    assert _count(owner["PinnedBuf"], "hipHostFree") == 1 and _count(owner["PinnedBuf"], "hipHostMalloc") == 1
    assert _count(fn["css_host_free"], "hipHostFree") == 1 and _count(fn["css_host_alloc"], "hipHostMalloc") == 1
    assert _count(fn["ensure"], "hipMalloc") == 1 and _count(fn["dev_alloc"], "hipMalloc") == 1
    # the owners cannot be copied: a copy would be a second release of the same resource
    for name, body in owner.items():
        assert re.search(rf"{name}\s*\(\s*const {name}\s*&\s*\)\s*=\s*delete", body), name
        assert re.search(rf"operator=\s*\(\s*const {name}\s*&\s*\)\s*=\s*delete", body), name
