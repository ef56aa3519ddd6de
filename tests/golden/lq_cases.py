"""LatentQuantize fixture configurations (shared by make_golden_lq.py and the LatentQuantize tests).

Every case builds LatentQuantize(**kwargs) (fixture tests/golden/data/lq_<name>.npz).  shape is the input's, always
channel-first [b, dim, ...]; train False = eval mode; x_scale multiplies the randn input; on_values: the leading positions
of batch 0 sit exactly on every value of every table; tables: "unsorted" / "dup" / "nan" overwrite the value tables
through load_state_dict before the forward (a shuffled table; a table with repeated values, where a tie goes to the
first; a NaN inside a table); nonfinite: positions 0 / 1 / 2 of batch 0 hold a NaN, +inf and -inf.  Cases with
projections are drawn until the two smallest distances of every projected value differ by at least 1e-4.
"""

LQ_CASES = {
    "seq": dict(kwargs=dict(levels=[5, 5, 8], dim=3), shape=[2, 3, 40]),
    "flat": dict(kwargs=dict(levels=[5, 5, 8], dim=3), shape=[24, 3]),
    "img": dict(kwargs=dict(levels=[5, 5, 8], dim=3), shape=[2, 3, 6, 5]),
    "proj": dict(kwargs=dict(levels=[5, 5, 8], dim=4), shape=[2, 4, 32]),
    "proj_555": dict(kwargs=dict(levels=[5, 5, 5], dim=4), shape=[2, 4, 32]),
    "int5": dict(kwargs=dict(levels=5, dim=4, codebook_dim=3), shape=[2, 4, 32]),
    "int5_noproj": dict(kwargs=dict(levels=5, dim=3, codebook_dim=3), shape=[2, 3, 32]),
    "novalues": dict(kwargs=dict(levels=[5, 5, 8], dim=3, optimize_values=False), shape=[2, 3, 40]),
    "novalues_proj": dict(kwargs=dict(levels=[5, 5, 8], dim=4, optimize_values=False), shape=[2, 4, 32]),
    "l6_7_10_11": dict(kwargs=dict(levels=[6, 7, 10, 11], dim=4), shape=[2, 4, 60], x_scale=0.5, on_values=True),
    "l15_22_24": dict(kwargs=dict(levels=[15, 22, 24], dim=3), shape=[2, 3, 60], x_scale=0.5, on_values=True),
    "l15": dict(kwargs=dict(levels=[15], dim=1), shape=[2, 1, 40], x_scale=0.5, on_values=True),
    "l26": dict(kwargs=dict(levels=[26], dim=1), shape=[2, 1, 40], x_scale=0.5, on_values=True),
    "d7": dict(kwargs=dict(levels=[3, 4, 5, 6, 7, 4, 3], dim=7), shape=[2, 7, 40], x_scale=0.5),
    "d8": dict(kwargs=dict(levels=[8, 5, 5, 5, 3, 3, 4, 6], dim=8), shape=[2, 8, 60]),
    "d16": dict(kwargs=dict(levels=[2] * 8 + [3] * 8, dim=16), shape=[2, 16, 40]),
    "unsorted": dict(kwargs=dict(levels=[5, 5, 8], dim=3), shape=[2, 3, 40], tables="unsorted", x_scale=0.5),
    "dup": dict(kwargs=dict(levels=[5, 5, 8], dim=3), shape=[2, 3, 40], tables="dup", x_scale=0.5, on_values=True),
    "nonfinite": dict(kwargs=dict(levels=[5, 5, 8], dim=3), shape=[1, 3, 20], nonfinite=True),
    "table_nan": dict(kwargs=dict(levels=[5, 5, 8], dim=3), shape=[1, 3, 20], tables="nan"),
    "w025_01": dict(kwargs=dict(levels=[5, 5, 8], dim=3, commitment_loss_weight=0.25, quantization_loss_weight=0.1),
                    shape=[2, 3, 40]),
    "w025_01_img": dict(kwargs=dict(levels=[6, 7, 10, 11], dim=4, commitment_loss_weight=0.25, quantization_loss_weight=0.1),
                        shape=[2, 4, 5, 6], x_scale=0.5),
    "w0": dict(kwargs=dict(levels=[5, 5, 8], dim=3, commitment_loss_weight=0.0, quantization_loss_weight=0.0),
               shape=[2, 3, 40]),
    "w_proj": dict(kwargs=dict(levels=[5, 5, 8], dim=4, commitment_loss_weight=0.25, quantization_loss_weight=0.1),
                   shape=[2, 4, 32]),
    "eval": dict(kwargs=dict(levels=[5, 5, 8], dim=3), shape=[2, 3, 40], train=False),
    "eval_proj": dict(kwargs=dict(levels=[5, 5, 8], dim=4), shape=[2, 4, 32], train=False),
}
