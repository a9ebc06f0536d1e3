"""Recipe for oracle/_ref/libtdv_ref_kernels.so — TEST INFRASTRUCTURE ONLY.

The reference's GPU half (cuda/depth_processing.cu, cuda/pointcloud.cu, cuda/icp.cu) includes nothing but
<cuda_runtime.h>.  With the name mapping of oracle/ref_shim/cuda_runtime.h on the include path, hipcc compiles the three
files for gfx950 straight from the reference tree, unchanged, into one shared library that exports the five launchers
(launchDepthPreprocess, launchBilateralFilter, launchDeproject, launchFindCorrespondences, launchBuildLinearSystem).
oracle/refkernels.py calls them; tests/test_gpu_reference_kernels.py holds the product's kernels to them.

-ffp-contract=off: the reference's sources do not fix contraction, the product library is built without it, and only
that build can be compared bit for bit.  Nothing else is chosen: -O3 and correctly rounded division are hipcc's
defaults for a release build.

The reference tree is read from TDV_REFERENCE_DIR (default /root/reference).  Nothing of it, and nothing compiled from it,
is committed: oracle/_ref/ is ignored by git.  The Eigen / OpenCV half (src/registration.cpp, src/pipeline.cpp) still
cannot be built here; see DESIGN.md section 2.
"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "_ref")
LIB = os.path.join(OUT_DIR, "libtdv_ref_kernels.so")
SHIM = os.path.join(HERE, "ref_shim")
SOURCES = ("cuda/depth_processing.cu", "cuda/pointcloud.cu", "cuda/icp.cu")
LAUNCHERS = ("launchDepthPreprocess", "launchBilateralFilter", "launchDeproject", "launchFindCorrespondences",
             "launchBuildLinearSystem")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-x", "hip", "-DCUDA_AVAILABLE", "-O3", "-fPIC", "-shared", "-ffp-contract=off"]


def reference_dir():
    return os.environ.get("TDV_REFERENCE_DIR", "/root/reference")


def have_reference():
    return all(os.path.isfile(os.path.join(reference_dir(), s)) for s in SOURCES)


def mangled_names(path=LIB):
    """{plain launcher name: its mangled export}, read from the library's own string table: the Itanium name of
    industry_picking::cuda::<name>(...) starts with the two namespaces and the length-prefixed plain name."""
    with open(path, "rb") as f:
        blob = f.read()
    out = {}
    for name in LAUNCHERS:
        found = set(re.findall(rb"_ZN16industry_picking4cuda%d%sE[A-Za-z0-9_]+" % (len(name), name.encode()), blob))
        if len(found) != 1:
            raise RuntimeError("%s: expected one export of %s, found %s" % (path, name, sorted(found)))
        out[name] = found.pop().decode()
    return out


def build(force=False):
    """Compile the library when the reference tree is present and the library is older than its inputs.  Returns the
    library's path, or None when there is no reference tree (oracle/_ref/ is then left as it is)."""
    if not have_reference():
        return None
    srcs = [os.path.join(reference_dir(), s) for s in SOURCES]
    deps = srcs + [os.path.join(SHIM, "cuda_runtime.h"), os.path.abspath(__file__)]
    if not force and os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    os.makedirs(OUT_DIR, exist_ok=True)
    tmp = LIB + ".tmp%d" % os.getpid()
    r = subprocess.run([HIPCC] + FLAGS + ["-I", SHIM] + srcs + ["-o", tmp], capture_output=True, text=True)
    if r.returncode != 0:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise RuntimeError("hipcc failed on the reference's kernels:\n" + r.stderr)
    mangled_names(tmp)
    os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    path = build(force="--force" in sys.argv)
    print(path if path else "no reference tree at %s: oracle/_ref/ left as it is" % reference_dir())
