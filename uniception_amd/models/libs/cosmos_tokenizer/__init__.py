"""The part of the Cosmos image tokenizer (reference: libs/cosmos_tokenizer) that CosmosEncoder and CosmosFeature stand on: the
continuous-image ("CI") encoder and decoder on the HIP kernels.  The video, discrete and JIT parts of the reference are not reproduced."""
