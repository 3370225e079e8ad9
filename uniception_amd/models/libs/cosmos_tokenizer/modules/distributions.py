"""Continuous formulations (reference: modules/distributions.py).  Only the autoencoder's identity has a HIP path; the VAE's sampling is
kept as a name so that a config can be built and refused with a message (CosmosEncoder.check_supported)."""
import torch


class IdentityDistribution(torch.nn.Module):
    "latent = the encoder's output; the second element mirrors the reference's (mean, logvar) placeholder"

    def forward(self, parameters):
        return parameters, (torch.tensor([0.0]), torch.tensor([0.0]))


class GaussianDistribution(torch.nn.Module):
    "mean + exp(logvar / 2) * noise: no HIP path (a random draw per latent element)"

    def __init__(self, min_logvar: float = -30.0, max_logvar: float = 20.0):
        super().__init__()
        self.min_logvar = min_logvar
        self.max_logvar = max_logvar

    def forward(self, parameters):
        from ....._lib import UcHipError
        raise UcHipError("GaussianDistribution: the VAE formulation has no HIP path (supported: 'AE')")
