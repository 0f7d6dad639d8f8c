"""Rank body of tests/test_ddp_lifecycle_gpu.py::test_accumulation_round_two_rccl_ranks (started by torch.distributed.run, one process per
GPU): ModelCross "tiny", batch sharded over the ranks, deterministic gradients, fp32 wire, gradient sink on.  Two backward + finish()
rounds on two batches with p.grad kept in between.  Saves, per rank, the local gradients of both rounds (taken without the reducer) and
p.grad after each round."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cross-attention-vit_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def main():
    out_dir, per_rank = sys.argv[1], int(sys.argv[2])
    rank, local, world = int(os.environ["RANK"]), int(os.environ["LOCAL_RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    import ref_cpu as R
    import xvit
    import xvit.functional as XF
    from xvit import ops
    from xvit.ddp import BucketedGradReducer
    ops.set_deterministic(True)
    cfg = R.make_config("tiny")
    model = xvit.ModelCross(cfg).to(dev)
    model.load_state_dict(R.make_state_dict(cfg, seed=0))
    model.train()
    sl = slice(rank * per_rank, (rank + 1) * per_rank)
    batches = [tuple(t[sl].to(dev) for t in R.make_inputs(cfg, per_rank * world, seed=s)) for s in (3, 8)]

    def grads():
        return {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}

    local_grads = []
    for img, labels in batches:                          # no reducer yet: this rank's own gradients (deterministic: the rounds below repeat them)
        for p in model.parameters():
            p.grad = None
        model(img, labels)[1].backward()
        torch.cuda.synchronize()
        local_grads.append(grads())
    red = BucketedGradReducer(list(model.parameters()), bucket_bytes=64 << 10, comm_dtype=torch.float32)
    XF.GRAD_SINK = red.grad_sink(model)
    red.zero_grad()
    after = []
    for img, labels in batches:
        model(img, labels)[1].backward()
        red.finish()
        torch.cuda.synchronize()
        after.append(grads())
    XF.GRAD_SINK = None
    torch.save({"local": local_grads, "after": after}, os.path.join(out_dir, f"a{rank}.pt"))
    if rank == 0:
        print(f"rccl ranks: {dist.get_world_size()} buckets: {len(red.buckets)}", flush=True)
    red.remove()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
