"""Tensor-level wrappers over the C-ABI.  PyTorch is used for device memory and streams only.

One module per operator family; ``_call`` holds what they share.  Everything is reached as ``ops.<name>``: product modules look a wrapper up on this
package when they call it (and so do the families among themselves), which is what lets a test replace one by assigning to the package attribute."""
from ._call import (_SD_DTYPES, _geom, _geom2d, _geom_cl, _pair, _triple,  # noqa: F401
                    augment_launch_count, cc_launch_count, prep_launch_count, resample_launch_count, sd_launch_count, seg_loss_launch_count,
                    tiles_launch_count, zoom2d_launch_count)
from ._call import ptr_struct as _ptr_struct  # noqa: F401  (the name scripts/ knew it by)
from .augment import (augment_channel_stats, augment_gaussian, augment_pointwise, augment_spatial, augment_spatial2d,  # noqa: F401
                      augment_spatial2d_labels, augment_spatial_labels, augment_spline_coefficients, augment_spline_coefficients2d)
from .blocks import (autocast_activation_dtype, lka2d_attention_backward, lka2d_attention_forward, lka2d_bf16_supported,  # noqa: F401
                     lka2d_saved_offsets, lka3d_attention_backward, lka3d_attention_forward, lka3d_attention_tokens_backward,
                     lka3d_attention_tokens_forward, lka3d_tokens_saved_offsets, lka3d_tokens_supported, tblock3d_backward, tblock3d_forward,
                     tblock3d_lka_bf16_supported, tblock3d_saved_activation_signs, tblock3d_saved_offsets, tblock3d_supported)
from .channels_last import (batchnorm_cl_backward, batchnorm_cl_forward, channel_scale, conv3d_backward_cl, conv3d_forward_cl,  # noqa: F401
                            deform_cl_grad_dtype, deform_conv3d_backward_cl, deform_conv3d_forward_cl, layernorm_tokens_backward,
                            layernorm_tokens_forward, ncdhw_to_ndhwc, ndhwc_to_ncdhw, scale_residual_backward, scale_residual_forward)
from .deform import (deform_conv2d_backward, deform_conv2d_forward, deform_conv2d_sample_index, deform_conv3d_backward,  # noqa: F401
                     deform_conv3d_forward, deform_conv3d_sample_index, deform_dwconv2d_backward_cl, deform_dwconv2d_forward_cl)
from .evaluation import (cc_component_table, cc_components, sd_distances, sd_label_stats, seg_eval_counts, seg_loss_backward,  # noqa: F401
                         seg_loss_forward)
from .inference import (tiles_blend, tiles_finalize, tiles_gather, zoom2d_argmax, zoom2d_coefficients, zoom2d_index_tables,  # noqa: F401
                        zoom2d_nearest, zoom2d_spline, zoom2d_spline_tables)
from .planar import (PLANAR_BN_STATS_ROWS, PLANAR_PW_CIN, batchnorm_planar_backward, batchnorm_planar_forward, conv3d_backward,  # noqa: F401
                     conv3d_forward, gelu_backward, gelu_forward, pointwise_planar_backward, pointwise_planar_forward,
                     pointwise_planar_supported)
from .prep import PREP_SCHEMES, _prep_desc, prep_crop, prep_mask_bbox, prep_nonzero_mask, prep_normalize  # noqa: F401
from .resample import (resample_argmax, resample_labels, resample_linear, resample_spline, spline_coefficients,  # noqa: F401
                       spline_prefilter)
