"""CPU: the PCA training entries of the C ABI (include/cvtmi.h, "PCA training") are exported and declared in plain C,
and the pca_train tool (pca_train_project/train/src/train.cpp) prints its usage without arguments.  No GPU involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
SYMBOLS = ["cvtmi_pca_covariance", "cvtmi_pca_covariance_dev", "cvtmi_pca_train", "cvtmi_pca_train_dev"]


def test_library_exports_training_entries():
    import cvt_amd
    lib = cvt_amd.lib()
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def test_header_declarations_compile_as_c99(tmp_path):
    src = tmp_path / "pca_train_decl.c"
    src.write_text('#include "cvtmi.h"\n'
                   "int main(void)\n{\n"
                   "    int (*a)(const float *, int64_t, int, float *, double *) = cvtmi_pca_covariance;\n"
                   "    int (*b)(const float *, int64_t, int, float *, double *, void *) = cvtmi_pca_covariance_dev;\n"
                   "    int (*c)(const float *, int64_t, int, int, float *, float *, float *) = cvtmi_pca_train;\n"
                   "    int (*d)(const float *, int64_t, int, int, float *, float *, float *, void *) = cvtmi_pca_train_dev;\n"
                   "    return (a && b && c && d) ? CVTMI_OK : CVTMI_EINVAL;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                   check=True)


def test_pca_train_usage():
    exe = os.path.join(BIN, "pca_train")
    assert os.path.exists(exe), "host CLIs not built: __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "usage: pca_train <feats.txt> <out.yml> [dim=2048] [num_reduced_dim=256]" in r.stdout
