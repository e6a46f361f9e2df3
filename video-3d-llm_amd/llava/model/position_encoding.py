"""llava.model.position_encoding on HIP: PositionEmbeddingSine3D (reference: position_encoding.py:5-49) and PositionEmbeddingMLP (:52-84)."""
import torch
import torch.nn as nn

from v3d import ops


class PositionEmbeddingSine3D(nn.Module):
    """Same constructor and call contract as the reference module; forward launches v3d_sin3d_pe, or v3d_sin3d_pe_points for
    n_points > 1 (the sample9 / sample5 / minmax types: x [B,N,P,3] -> [B,N,E])."""

    def __init__(self, embedding_size, temperature=10000, n_points=1):
        super().__init__()
        self.embedding_size = embedding_size
        self.temperature = temperature
        self.n_points = n_points
        # the reference recomputes this on every call (position_encoding.py:24-25); same torch expression, once
        self._dim_t = ops.reference_dim_t(embedding_size // (3 * n_points), temperature)
        self._dim_t_dev = {}

    def forward(self, x):
        key = x.device
        if key not in self._dim_t_dev:
            self._dim_t_dev[key] = self._dim_t.to(x.device)
        return ops.sin3d_pe(x, self.embedding_size, dim_t=self._dim_t_dev[key], n_points=self.n_points)


class PositionEmbeddingMLP(nn.Module):
    """Same constructor, parameter names (mlp.0 / mlp.1 / mlp.3) and call contract as the reference module: x [B,N,3] -> [B,N,E] in x's
    dtype.  forward launches v3d_pe_mlp_hidden (Linear(3, 512), LayerNorm, ReLU) and v3d_gemm (Linear(512, E)); the parameters must be on
    the device in x's 16-bit dtype.  n_points > 1 is refused: the reference's forward names an undefined `num_feats` there (:79)."""

    def __init__(self, embedding_size, temperature=10000, n_points=1):
        super().__init__()
        if n_points != 1:
            raise NotImplementedError("PositionEmbeddingMLP with n_points > 1 does not run in the reference (position_encoding.py:79)")
        self.embedding_size = embedding_size
        self.temperature = temperature
        self.n_points = n_points
        self.hidden_size = ops.PE_MLP_HIDDEN
        self.mlp = nn.Sequential(nn.Linear(3, self.hidden_size), nn.LayerNorm(self.hidden_size), nn.ReLU(),
                                 nn.Linear(self.hidden_size, self.embedding_size))

    def tensors(self):
        m = self.mlp
        return {"w0": m[0].weight.data, "b0": m[0].bias.data, "ln_w": m[1].weight.data, "ln_b": m[1].bias.data, "w3": m[3].weight.data,
                "b3": m[3].bias.data}

    def forward(self, x):
        B, N, _ = x.shape
        return ops.pe_mlp(x, self.tensors()).view(B, N, self.embedding_size)
