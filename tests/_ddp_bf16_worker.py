"""Rank body of tests/test_grad_comm_gpu.py::test_bf16_reducer_two_rccl_ranks (started by torch.distributed.run, one process per GPU):
ModelCross "tiny", batch sharded over the ranks, deterministic gradients.  Reduces the same step-0 gradients through an fp32 and a bf16
reducer, then takes 3 Adam steps through the bf16 reducer.  Saves the local and the reduced gradients of both and the final parameters
per rank."""
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
    from xvit import ops
    from xvit.ddp import BucketedGradReducer
    ops.set_deterministic(True)
    cfg = R.make_config("tiny")
    torch.manual_seed(1000 + rank)                       # different init per rank: the reducer's broadcast must fix it
    model = xvit.ModelCross(cfg).to(dev)
    if rank == 0:
        model.load_state_dict(R.make_state_dict(cfg, seed=0))
    model.train()
    img, labels = R.make_inputs(cfg, per_rank * world, seed=3)
    sl = slice(rank * per_rank, (rank + 1) * per_rank)
    img, labels = img[sl].to(dev), labels[sl].to(dev)

    def reduced(red):
        """(this rank's local gradients, the reduced ones); no gradient sink: p.grad stays the local tensor until finish()"""
        red.zero_grad()
        _, loss = model(img, labels)
        loss.backward()
        torch.cuda.synchronize()
        local = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
        red.finish()
        torch.cuda.synchronize()
        return local, {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}

    red32 = BucketedGradReducer(list(model.parameters()), bucket_bytes=64 << 10, comm_dtype=torch.float32)
    l32, g32 = reduced(red32)
    red32.remove()
    red = BucketedGradReducer(list(model.parameters()), bucket_bytes=64 << 10, comm_dtype=torch.bfloat16, broadcast=False)
    l16, g16 = reduced(red)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for _ in range(3):
        reduced(red)
        opt.step()
    torch.cuda.synchronize()
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    torch.save({"l32": l32, "l16": l16, "g32": g32, "g16": g16, "params": params}, os.path.join(out_dir, f"w{rank}.pt"))
    if rank == 0:
        print(f"rccl ranks: {dist.get_world_size()} buckets: {len(red.buckets)}", flush=True)
    red.remove()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
