# Top-level build for C users, through the Python build in cuda_satabsearch_amd/build.py:
#   make            libsatabsearch.so (HIP kernels + C ABI), libsathost.so (reader, statistics),
#                   cuda_satabsearch_amd/bin/satabsearch (command line)
#   make oracle     the CPU oracle used by the tests (oracle/), plus the reference build when
#                   /root/reference is mounted
#   make test       CPU test suite;  make test-gpu on a machine with an MI355X
# The sources, flags and dependencies of all three are cuda_satabsearch_amd/build.py's alone (DEVICE_SOURCES: one object
# per translation unit of the device library, re-made only when it or a header it includes changed: sat_launch.hip,
# sat_capi.hip, sat_pairs.hip, sat_db.hip, sat_topk.hip, sat_multi.hip, sat_polish.hip, sat_qfromdb.hip,
# sat_cluster.hip, sat_eval.hip, sat_cover.hip, sat_profile.hip, sat_reorder.hip, sat_exact.hip, sat_reach.hip; the host
# library's plain-C files, csrc/host/sat_exact.c and csrc/host/sat_reach.c among them, are build_host's list there).
PKG      = cuda_satabsearch_amd

all:
	python -m $(PKG).build

oracle:
	$(MAKE) -C oracle all
	if [ -d /root/reference/nvcc_src_current ]; then $(MAKE) -C oracle ref; fi

test: all oracle
	python -m pytest tests -q -m "not gpu"

test-gpu: all oracle
	python -m pytest tests -q -m gpu

clean:
	rm -f $(PKG)/libsathost.so $(PKG)/libsatabsearch.so $(PKG)/bin/satabsearch $(PKG)/*.o
	rm -rf $(PKG)/obj
	$(MAKE) -C oracle clean

.PHONY: all oracle test test-gpu clean
