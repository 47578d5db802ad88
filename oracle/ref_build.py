"""Recipe for oracle/_ref/: the reference compiled as C, as a second opinion beside oracle/liboracle.so.

    python oracle/ref_build.py            (build() of __graft_entry__.py calls build_ref())

The reference tree is $AOMHIP_REFERENCE_DIR (default /root/reference).  Where it does not exist the recipe does nothing and an existing
oracle/_ref/ stays as it is (a machine that received oracle/_ref/ ready-made).  Otherwise the tree is configured with cmake for the
`generic` CPU target in a temporary directory outside the repository, `aom` is built there with ninja, and libaom.a is linked whole
into oracle/_ref/libaomref_c.so, so every *_c function and every non-static encoder function is an exported symbol.  Every
oracle/refshim/*.c (our own text: flat-array entry points around reference functions that take structs) is compiled against the
reference's headers and that build's config/ directory into oracle/_ref/librefshim.so.  The temporary directory is removed: no object
tree and no generated header ever lies in the repository, and oracle/_ref/ is ignored by git.  oracle/_ref/MANIFEST.json records what
was built from what; when it matches, nothing is rebuilt."""
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
SHIMS = os.path.join(HERE, "refshim")
LIB = "libaomref_c.so"
SHIM_LIB = "librefshim.so"
JOBS = 16  # never sized by the machine's CPU count
CMAKE_OPTIONS = ["-G", "Ninja", "-DAOM_TARGET_CPU=generic", "-DENABLE_TESTS=0", "-DENABLE_EXAMPLES=0", "-DENABLE_DOCS=0",
                 "-DENABLE_TOOLS=0", "-DCMAKE_BUILD_TYPE=Release", "-DCMAKE_POSITION_INDEPENDENT_CODE=ON"]


def reference_dir():
    return os.environ.get("AOMHIP_REFERENCE_DIR", "/root/reference")


def _source_digest(ref):
    """sha256 over (relative name, size) of every .c / .h file of the reference tree, in sorted order."""
    h = hashlib.sha256()
    rows = []
    for top, dirs, files in os.walk(ref):
        dirs[:] = sorted(d for d in dirs if d != ".git")
        for f in files:
            if f.endswith((".c", ".h")):
                p = os.path.join(top, f)
                rows.append((os.path.relpath(p, ref), os.path.getsize(p)))
    for name, size in sorted(rows):
        h.update(("%s\0%d\n" % (name, size)).encode())
    return h.hexdigest(), len(rows)


def _shim_digest():
    h = hashlib.sha256()
    for p in sorted(glob.glob(os.path.join(SHIMS, "*.[ch]"))):
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _compiler_version():
    cc = os.environ.get("CC", "cc")
    out = subprocess.run([cc, "--version"], capture_output=True, text=True, check=True).stdout
    return out.splitlines()[0].strip()


def wanted_manifest(ref):
    digest, n = _source_digest(ref)
    return {"source_digest": digest, "source_files": n, "cmake_options": CMAKE_OPTIONS, "compiler": _compiler_version(),
            "shim_digest": _shim_digest(), "libraries": [LIB] + ([SHIM_LIB] if glob.glob(os.path.join(SHIMS, "*.c")) else [])}


def up_to_date(want):
    try:
        with open(os.path.join(OUT, "MANIFEST.json")) as f:
            have = json.load(f)
    except (OSError, ValueError):
        return False
    return have == want and all(os.path.exists(os.path.join(OUT, l)) for l in want["libraries"])


def _run(cmd, verbose):
    """a build step; its output is shown only with -v or when it fails"""
    if verbose:
        subprocess.check_call(cmd)
        return
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout)
        raise subprocess.CalledProcessError(r.returncode, cmd)


def build_ref(verbose=False):
    """Returns 'absent' (no reference tree: nothing done), 'current' (manifest matches: nothing done) or 'built'."""
    ref = reference_dir()
    if not os.path.isdir(ref):
        return "absent"
    want = wanted_manifest(ref)
    if up_to_date(want):
        return "current"
    cc = os.environ.get("CC", "cc")
    tmp = tempfile.mkdtemp(prefix="aomhip_ref_")
    try:
        bld, stage = os.path.join(tmp, "build"), os.path.join(tmp, "out")
        os.makedirs(bld)
        os.makedirs(stage)
        _run(["cmake", "-S", ref, "-B", bld] + CMAKE_OPTIONS, verbose)
        _run(["ninja", "-C", bld, "-j%d" % JOBS, "aom"], verbose)
        _run([cc, "-shared", "-o", os.path.join(stage, LIB), "-Wl,--whole-archive", os.path.join(bld, "libaom.a"),
              "-Wl,--no-whole-archive", "-lm", "-lpthread"], verbose)
        shims = sorted(glob.glob(os.path.join(SHIMS, "*.c")))
        if shims:
            # the shims resolve the reference's functions from libaomref_c.so beside them ($ORIGIN), one copy of its tables per process
            _run([cc, "-O2", "-fPIC", "-shared", "-std=gnu11", "-Wall", "-I" + ref, "-I" + bld, "-o", os.path.join(stage, SHIM_LIB)]
                 + shims + ["-L" + stage, "-laomref_c", "-Wl,-rpath,$ORIGIN", "-lm"], verbose)
        os.makedirs(OUT, exist_ok=True)
        for l in want["libraries"]:
            os.replace(shutil.copy(os.path.join(stage, l), os.path.join(OUT, l + ".tmp")), os.path.join(OUT, l))
        with open(os.path.join(OUT, "MANIFEST.json"), "w") as f:
            json.dump(want, f, indent=1, sort_keys=True)
            f.write("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return "built"


if __name__ == "__main__":
    print("oracle/_ref:", build_ref(verbose="-v" in sys.argv[1:]))
