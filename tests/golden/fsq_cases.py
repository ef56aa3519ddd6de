"""FSQ / ResidualFSQ / GroupedResidualFSQ fixture configurations (shared by make_golden_fsq.py and the FSQ tests).

kind "fsq" builds FSQ(**kwargs) (fixture tests/golden/data/fsq_<name>.npz), kind "rfsq" ResidualFSQ(**kwargs) and "grfsq"
GroupedResidualFSQ(**kwargs) (rfsq_<name>.npz).  shape is the input's (channel-last unless channel_first); dtype its
dtype (default float32); train False = eval mode; seed: the fixed quantize-dropout seed passed to ResidualFSQ.forward
(GroupedResidualFSQ draws its own from random.seed(py_seed)); codes: forward with return_all_codes=True; nonfinite: rows
0 / 1 / 2 hold a NaN, +inf and -inf; collide: the leading rows hit every code whose index term is not an integer.
"""

FSQ_CASES = {
    "l8555": dict(kind="fsq", kwargs=dict(levels=[8, 5, 5, 5]), shape=[2, 40, 4]),
    "l865": dict(kind="fsq", kwargs=dict(levels=[8, 6, 5]), shape=[2, 40, 3]),
    "l75555": dict(kind="fsq", kwargs=dict(levels=[7, 5, 5, 5, 5]), shape=[2, 40, 5]),
    "proj": dict(kind="fsq", kwargs=dict(levels=[8, 5, 5, 5], dim=16), shape=[2, 30, 16]),
    "img_cf": dict(kind="fsq", kwargs=dict(levels=[8, 5, 5, 5], channel_first=True), shape=[2, 4, 6, 5]),
    "c2_keep": dict(kind="fsq", kwargs=dict(levels=[8, 5, 5, 5], num_codebooks=2, keep_num_codebooks_dim=True),
                    shape=[2, 30, 8]),
    "noidx": dict(kind="fsq", kwargs=dict(levels=[8, 5, 5, 5], return_indices=False), shape=[2, 30, 4]),
    "f64": dict(kind="fsq", kwargs=dict(levels=[8, 5, 5, 5]), shape=[2, 30, 4], dtype="float64"),
    "bf16": dict(kind="fsq", kwargs=dict(levels=[8, 5, 5, 5]), shape=[2, 30, 4], dtype="bfloat16"),
    "nonfinite": dict(kind="fsq", kwargs=dict(levels=[8, 5, 5, 5]), shape=[1, 20, 4], nonfinite=True),
    "l26": dict(kind="fsq", kwargs=dict(levels=[26]), shape=[1, 60, 1], collide=True),
    "l27_5": dict(kind="fsq", kwargs=dict(levels=[27, 5]), shape=[1, 60, 2], collide=True),
    "l1000": dict(kind="fsq", kwargs=dict(levels=[1000]), shape=[1, 60, 1], collide=True),
}

RFSQ_CASES = {
    "q1": dict(kind="rfsq", kwargs=dict(dim=4, levels=[8, 5, 5, 5], num_quantizers=1), shape=[2, 30, 4]),
    "q3": dict(kind="rfsq", kwargs=dict(dim=4, levels=[8, 5, 5, 5], num_quantizers=3), shape=[2, 30, 4]),
    "q8": dict(kind="rfsq", kwargs=dict(dim=4, levels=[8, 5, 5, 5], num_quantizers=8), shape=[2, 20, 4]),
    "q3_865": dict(kind="rfsq", kwargs=dict(dim=3, levels=[8, 6, 5], num_quantizers=3), shape=[2, 30, 3]),
    "proj": dict(kind="rfsq", kwargs=dict(dim=16, levels=[8, 5, 5, 5], num_quantizers=3), shape=[2, 25, 16]),
    "eval": dict(kind="rfsq", kwargs=dict(dim=4, levels=[8, 5, 5, 5], num_quantizers=3), shape=[2, 30, 4], train=False),
    "drop_cut": dict(kind="rfsq", kwargs=dict(dim=4, levels=[8, 5, 5, 5], num_quantizers=6, quantize_dropout=True,
                                              quantize_dropout_cutoff_index=1), shape=[2, 25, 4], seed=3),
    "drop_m2": dict(kind="rfsq", kwargs=dict(dim=4, levels=[8, 5, 5, 5], num_quantizers=8, quantize_dropout=True,
                                             quantize_dropout_cutoff_index=1, quantize_dropout_multiple_of=2),
                    shape=[2, 25, 4], seed=11),
    "drop_full": dict(kind="rfsq", kwargs=dict(dim=4, levels=[8, 5, 5, 5], num_quantizers=4, quantize_dropout=True,
                                               quantize_dropout_cutoff_index=3), shape=[2, 25, 4], seed=1),
    "codes": dict(kind="rfsq", kwargs=dict(dim=4, levels=[8, 5, 5, 5], num_quantizers=3), shape=[2, 20, 4], codes=True),
    "g2": dict(kind="grfsq", kwargs=dict(dim=8, groups=2, levels=[8, 5, 5, 5], num_quantizers=3), shape=[2, 25, 8]),
    "g4": dict(kind="grfsq", kwargs=dict(dim=16, groups=4, levels=[8, 5, 5, 5], num_quantizers=3), shape=[2, 20, 16]),
    "g2_proj": dict(kind="grfsq", kwargs=dict(dim=32, groups=2, levels=[8, 5, 5, 5], num_quantizers=3), shape=[2, 20, 32]),
    "g4_proj": dict(kind="grfsq", kwargs=dict(dim=64, groups=4, levels=[8, 5, 5, 5], num_quantizers=2), shape=[1, 20, 64]),
    "g2_codes": dict(kind="grfsq", kwargs=dict(dim=8, groups=2, levels=[8, 5, 5, 5], num_quantizers=3), shape=[2, 15, 8],
                     codes=True),
    "g2_drop": dict(kind="grfsq", kwargs=dict(dim=8, groups=2, levels=[8, 5, 5, 5], num_quantizers=4,
                                              quantize_dropout=True), shape=[2, 15, 8], py_seed=2),
}
