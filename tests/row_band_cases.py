"""The (batch, workgroup target) pairs with which the GPU tests reach 1, 2, 4 and 8 row bands per image at a handful of images
(csrc/ian_row_bands.h: an image is halved while batch x bands < target).  tests/test_row_bands_host.py pins on the CPU that every pair
gives the band count it is listed under; tests/test_gpu_image_layers.py and tests/test_gpu_train_kernels.py sweep them."""

# {bands: value of the option}; the same value serves every batch listed beside it
DEC_OUT_BATCHES, DEC_OUT_WGS = (4, 5), {1: 1, 2: 8, 4: 16, 8: 32}          # dec_out_wgs, IAN_simple's dec_out (32 input rows, row pairs)
HEAD_BATCHES, HEAD_WGS = (3, 5), {1: 1, 2: 6, 4: 12, 8: 32}                # head_wgs, the RGB-Beta head (64 rows, halo 4)
TRAIN_HEAD_BATCH, TRAIN_HEAD_WGS = 2, {1: 1, 2: 4, 4: 8, 8: 256}           # head_wgs, ian_layer_head6_forward at 64 rows; 256 = the default
