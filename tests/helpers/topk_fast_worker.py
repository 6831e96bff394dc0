"""One rank of `evalrank_fast(model_path, split='test', topk=5)` over gloo (tests/test_topk_gpu.py starts two of them with
torch.distributed.run; both share this box's one GPU, the collectives are host-staged)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "image-text-retrieval_amd"))

import torch                                   # noqa: E402
import torch.distributed as dist               # noqa: E402

from itr_amd.metricmodule import evaluation    # noqa: E402

if __name__ == "__main__":
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    evaluation.evalrank_fast(sys.argv[1], split='test', topk=5)
    dist.destroy_process_group()
