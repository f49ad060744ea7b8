"""What a header declares and what a library exports, for the "exports exactly its header" tests of every library."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions(header):
    """The sorted ``tsdf_*`` function names that include/<header> declares (comments stripped)."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_\w+)\s*\(", text)))


def exported(path):
    """``(functions, named)`` of a shared library's dynamic symbols: every function it defines, and every defined symbol
    whose name starts with ``tsdf_``, both sorted."""
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    rows = [ln.split() for ln in out.splitlines() if ln.strip()]
    return sorted(r[-1] for r in rows if r[-2] in "TtWw"), sorted(r[-1] for r in rows if r[-1].startswith("tsdf_"))
