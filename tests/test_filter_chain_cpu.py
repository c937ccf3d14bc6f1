"""The filter chain of pcs-multicamera-optimized (pointcloud_stitching_amd/cli/pcs_filter_chain.h) without a GPU: tools/filter_chain_check.cpp
runs it over host-memory fakes of the library calls it makes — all 16 subsets of -O -K -M -E, from a host count and from a device
count — and checks which entry point every stage gets, with which pointers, counts and sizes, the returned cloud, the -t lines and
that every block is freed once. The plain build only: the sanitizer target of the same Makefile is run by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_DIR = os.path.join(ROOT, "pointcloud_stitching_amd", "cli")
CHECK = os.path.join(ROOT, "tools", "bin", "filter_chain_check")


def test_the_chain_over_fakes_of_the_library():
    made = subprocess.run(["make", "-C", CLI_DIR, "../../tools/bin/filter_chain_check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert made.returncode == 0, made.stdout
    ran = subprocess.run([CHECK], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout
    assert "all checks passed" in ran.stdout
