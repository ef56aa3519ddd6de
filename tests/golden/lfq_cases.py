"""LFQ fixture configurations (shared by make_golden_lfq.py and the LFQ tests).

kwargs go to the LFQ constructor; shape is the input's; tau the forward's inv_temperature; train False = eval mode;
mask: a [b, n] prefix mask (row i keeps n // (i + 2) rows); zeros: every zeros-th input element set to exactly 0.
"""

LFQ_CASES = {
    "d1": dict(kwargs=dict(codebook_size=2, dim=1), shape=[2, 33, 1], tau=1.0),
    "d4": dict(kwargs=dict(codebook_size=16, dim=4), shape=[3, 50, 4], zeros=7),
    "d4_eval": dict(kwargs=dict(codebook_size=16, dim=4), shape=[2, 40, 4], train=False),
    "d9_c2": dict(kwargs=dict(codebook_size=512, dim=18, num_codebooks=2), shape=[2, 37, 18], tau=1.0),
    "d9_proj": dict(kwargs=dict(codebook_size=512, dim=24), shape=[2, 45, 24], tau=1.0),
    "d9_cos": dict(kwargs=dict(codebook_size=512, dim=20, cosine_sim_project_in=True), shape=[2, 30, 20], tau=1.0),
    "d12": dict(kwargs=dict(codebook_size=4096, dim=12), shape=[2, 61, 12], x_scale=0.05),
    "d12_sph": dict(kwargs=dict(codebook_size=4096, dim=12, spherical=True), shape=[2, 40, 12], tau=10.0),
    "d12_clamp": dict(kwargs=dict(codebook_size=4096, dim=12, soft_clamp_input_value=2.0, codebook_scale=1.5),
                      shape=[2, 40, 12], tau=1.0),
    "d12_mask": dict(kwargs=dict(codebook_size=4096, dim=12), shape=[3, 40, 12], mask=True, tau=1.0),
    "d12_frac": dict(kwargs=dict(codebook_size=4096, dim=12, frac_per_sample_entropy=0.5), shape=[2, 50, 12], tau=1.0),
    "d12_softplus": dict(kwargs=dict(codebook_size=4096, dim=12, experimental_softplus_entropy_loss=True,
                                     diversity_gamma=0.5), shape=[2, 40, 12], tau=1.0),
    "d12_img": dict(kwargs=dict(codebook_size=4096, dim=12, channel_first=True), shape=[2, 12, 5, 7], tau=1.0),
    "d4_c2_img": dict(kwargs=dict(codebook_size=16, dim=12, num_codebooks=2, channel_first=True), shape=[2, 12, 3, 4],
                      tau=1.0),
    "d16": dict(kwargs=dict(codebook_size=65536, dim=16), shape=[1, 24, 16], tau=1.0),
    "d16_t100": dict(kwargs=dict(codebook_size=65536, dim=16), shape=[1, 16, 16], x_scale=0.001),
    "d16_c2_nocommit": dict(kwargs=dict(codebook_size=65536, dim=32, num_codebooks=2, commitment_loss_weight=0.0),
                            shape=[1, 8, 32], tau=1.0),
}
