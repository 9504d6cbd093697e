"""Pose head, ``PW/pose_calculator.py:20-87``: masked sum over points -> 64->256 -> (q, t)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..pointnet2_ops.pytorch_utils import Conv1d


class PoseCalculator(nn.Module):
    """(embedding_features (B,C,N), mask (B,C,N)) -> q (B,4[,1]) unit quaternion, t (B,3[,1])."""

    def __init__(self, in_channel: int, out_channel: int, kernel_size: int = 1, padding="valid",
                 activation=None, pose=None, squeeze: bool = True, bn_decay=None):
        super().__init__()
        self.pose = pose
        self.squeeze = squeeze
        xavier = torch.nn.init.xavier_uniform_
        kw = dict(kernel_size=kernel_size, padding=padding, activation=activation, init=xavier)
        self.conv1d_q_t = Conv1d(in_size=in_channel, out_size=out_channel, **kw)
        self.conv1d_q = Conv1d(in_size=out_channel, out_size=4, **kw)
        self.conv1d_t = Conv1d(in_size=out_channel, out_size=3, **kw)

    def forward(self, embedding_features, mask):
        pooled = torch.sum(embedding_features * mask, dim=2, keepdim=True)
        big = self.conv1d_q_t(pooled)
        big_q = F.dropout(big, p=0.5, training=self.training)
        big_t = F.dropout(big, p=0.5, training=self.training)
        q = self.conv1d_q(big_q)
        q = q / (torch.sqrt(torch.sum(q * q, dim=1, keepdim=True) + 1e-10) + 1e-10)
        t = self.conv1d_t(big_t)
        if self.squeeze:
            q, t = q.squeeze(2), t.squeeze(2)
        return q, t

    def from_logits(self, embedding_features, mask_logits):
        """``self(embedding_features, F.softmax(mask_logits, dim=2))`` -- exactly that while no
        ``training.DropoutStream`` is attached, in ``eval()`` and for tensors the kernels do not cover.  With a stream
        attached and in ``train()`` mode the whole head, soft-max included, is one hand-written kernel pair each way
        (``..pose_head``) and its two dropout masks come from the stream's counter-based generator."""
        attached = getattr(self, "_dropout_stream", None)
        if attached is not None and self.training:
            from .. import pose_head
            stream, head = attached
            qt, q_, t_ = self.conv1d_q_t.conv, self.conv1d_q.conv, self.conv1d_t.conv
            weights = (qt.weight, qt.bias, q_.weight, q_.bias, t_.weight, t_.bias)
            if pose_head.supported(embedding_features, mask_logits, weights):
                q, t, _keep = pose_head.pose_head_train(embedding_features, mask_logits, *weights, stream.state_on(
                    embedding_features.device), stream.rank, head, stream.keep_log(head, embedding_features.shape[0],
                                                                                  embedding_features.device))
                return (q, t) if self.squeeze else (q.unsqueeze(2), t.unsqueeze(2))
        return self(embedding_features, F.softmax(mask_logits, dim=2))
