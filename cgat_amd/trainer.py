"""One data-parallel training step of the reference harness on this path (BASELINE configs[3]):

    LightningModel.training_step / evaluate / configure_optimizers        CGAT/lightning_module.py:185-259, 306-355
    Trainer(strategy='ddp', accumulate_grad_batches=...)                  CGAT/train.py:53-79

collate the rank's crystals on the device (PackedDataset) -> CGAtNet forward -> `.chunk(2, dim=1)` into
(output, log_std) -> criterion against the normalised target, with the step's mae / rmse, in one launch -> backward with
the bucketed gradient all-reduce overlapped (GradientAverager: RCCL over xGMI) -> one fused optimiser step (`optim=`:
SGD, Adam, AdamW or LAMB, lightning_module.py:319-338).  Nothing here touches the host per crystal; per step the host
uploads the batch's crystal ids and three prefix sums.
"""
import numpy as np
import torch

from .dist import GradientAverager, shard_range
from .optim import FusedAdam, FusedAdamW, FusedLamb, FusedSGD, criterion_with_metrics


class Normalizer:
    """target -> (target - mean) / std and back (CGAT/utils.py Normalizer as used at lightning_module.py:205-211)."""

    def __init__(self, mean=0.0, std=1.0):
        self.mean, self.std = float(mean), float(std)

    def norm(self, t):
        return (t - self.mean) / self.std

    def denorm(self, t):
        return t * self.std + self.mean


class DataParallelTrainer:
    def __init__(self, model, dataset, lr=1e-3, weight_decay=1e-2, loss="L1", normalizer=None, accumulate_grad_batches=1,
                 rank=0, world=1, bucket_bytes=64 << 20, force_averager=False, static_graph=True, optim="AdamW",
                 momentum=0.9, std_loss=False, only_residual=False):
        self.model, self.dataset = model, dataset
        self.rank, self.world = rank, world
        self.params = [p for p in model.parameters() if p.requires_grad]
        # only_residual: the optimiser sees the output network alone (lightning_module.py:314-317); gradients are still
        # formed and all-reduced for every parameter, as in the reference
        trained = [p for p in model.get_output_parameters() if p.requires_grad] if only_residual else self.params
        if optim == "SGD":
            self.optimizer = FusedSGD(trained, lr=lr, weight_decay=weight_decay, momentum=momentum)
        elif optim == "Adam":
            self.optimizer = FusedAdam(trained, lr=lr, weight_decay=weight_decay)
        elif optim == "AdamW":
            self.optimizer = FusedAdamW(trained, lr=lr, weight_decay=weight_decay)
        elif optim == "LAMB":
            self.optimizer = FusedLamb(trained, lr=lr, weight_decay=weight_decay)
        else:
            raise NameError("Only SGD, Adam, AdamW, LAMB are allowed as optim")
        # static_graph: the set of never-used parameters is fixed by the architecture (Edge.MH_A / Edge.MH_M under
        # no_hyper=True), so the averager may freeze it after two steps and stop synchronising with the host
        # force_averager: the bucketed all-reduce also at world size 1 (a one-rank RCCL communicator; dist.GradientAverager)
        # (created only when it will be active: force=True without a process group raises in GradientAverager)
        self.averager = (GradientAverager(self.params, bucket_bytes=bucket_bytes, force=force_averager, static_graph=static_graph)
                         if (world > 1 or force_averager) else None)
        # std_loss: nn.L1Loss / nn.MSELoss instead of the robust losses (lightning_module.py:131-142)
        self.criterion = ("" if std_loss else "Robust") + ("L1" if loss == "L1" else "L2")
        self.normalizer = normalizer or Normalizer()
        self.accumulate = int(accumulate_grad_batches)
        self.last_metrics = None

    def local_ids(self, global_ids):
        """This rank's contiguous share of a global batch of crystal ids (graphs are independent: no halo)."""
        lo, hi = shard_range(len(global_ids), self.rank, self.world)
        return np.asarray(global_ids)[lo:hi]

    def _evaluate(self, ids):
        """Loss against the normalised target, mae and rmse of the de-normalised prediction (lightning_module.py:206-210,
        240-243): device tensors of this rank's batch."""
        batch, roost = self.dataset.collate(ids)
        output, log_std = self.model(batch, roost).chunk(2, dim=1)
        loss, mae, rmse = criterion_with_metrics(self.criterion, output, log_std, batch.y.view(-1, 1),
                                                 self.normalizer.mean, self.normalizer.std)
        return loss, mae, rmse, batch

    def _loss(self, ids):
        loss, mae, rmse, batch = self._evaluate(ids)
        self.last_metrics = {"loss": loss.detach(), "mae": mae, "rmse": rmse}
        return loss, batch

    def validate(self, ids):
        """(loss, mae, rmse) of this rank's crystals `ids` in eval mode without grad (validation_step / test_step,
        lightning_module.py:261-301), so the node layers take their no-grad forward.  Touches no gradient and no optimiser
        state; the model's training mode is restored.  Per rank: averaging over ranks is the caller's."""
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                loss, mae, rmse, _ = self._evaluate(ids)
        finally:
            self.model.train(was_training)
        return loss, mae, rmse

    def step(self, ids):
        """`ids`: this rank's crystal ids for the step (or a list of `accumulate_grad_batches` id arrays).
        Returns (loss, edges processed on this rank); `loss` is the last micro-batch's criterion divided by the number of
        micro-batches, i.e. the term that was back-propagated.  `self.last_metrics` holds the last micro-batch's
        {"loss", "mae", "rmse"} as device tensors, `loss` there being the criterion itself, undivided, as the harness logs
        it; the two are the same tensor value at `accumulate_grad_batches=1`.  The gradient is the kernel's mean-loss
        gradient times the incoming 1 / micro-batches: at `accumulate_grad_batches=1` (and any power of two) that is the
        robust losses' own gradient bit for bit, otherwise it may differ from it in the last place."""
        micro = list(ids) if self.accumulate > 1 else [ids]
        if self.averager is not None:
            self.averager.zero_grad()                  # gradients accumulate straight into the all-reduce buckets
        else:
            for p in self.params:
                p.grad = None
        edges = 0
        for k, mb in enumerate(micro):
            last = k == len(micro) - 1
            loss, batch = self._loss(mb)
            loss = loss / len(micro)
            if self.averager is not None and not last:
                with self.averager.no_sync():
                    loss.backward()
            else:
                loss.backward()
            edges += int(batch.edge_index.shape[1])
        if self.averager is not None:
            self.averager.finish()
        self.optimizer.step()
        return loss.detach(), edges
