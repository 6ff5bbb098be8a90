"""The torch half of tests/test_gpu_caller_stream.py, as a process of its own:

    python tests/torch_stream_child.py OUT.npz RESTARTS FIRST_ORDINAL

torch is imported before the device library, as bench.py does it, so that both use one HIP runtime.  On torch's default
stream ("current") and inside `with torch.cuda.stream(torch.cuda.Stream())` ("side"): use_stream(torch's current stream),
search_async with LORDER, a clone of device_scores_tensor() with nothing synchronised, search_async without LORDER,
torch.cuda.synchronize().  Writes {where}_clone and {where}_results; the test holds them against the oracle."""
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import cuda_satabsearch_amd as sat  # noqa: E402
import stream_lib  # noqa: E402  (beside this file: the script's directory is on sys.path)


def main(out, restarts, first):
    if not torch.cuda.is_available():
        raise RuntimeError("torch sees no GPU")
    db, queries = stream_lib.world_inputs()
    rows = {}
    with sat.Searcher(0) as s:
        s.upload(db)
        s.set_queries(queries, first)
        for where in ("current", "side"):
            with (torch.cuda.stream(torch.cuda.Stream()) if where == "side" else contextlib.nullcontext()):
                s.use_stream(torch.cuda.current_stream().cuda_stream)
                s.search_async(False, False, 1)             # the descriptors are made: nothing below waits on the host
                s.sync()
                s.search_async(True, False, restarts)
                clone = s.device_scores_tensor().clone()
                s.search_async(False, False, restarts)
                assert s.last_launch_info().count(";") + 1 >= 2
                torch.cuda.synchronize()
                rows[where + "_clone"] = clone.cpu().numpy()
                rows[where + "_results"] = s.results()[0]
                s.use_own_stream()
    np.savez(out, **rows)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
