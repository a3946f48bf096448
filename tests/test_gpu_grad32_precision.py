"""GPU (-m gpu): the TRAINING-time entries of the fp32 kernels -- forward, input gradient, weight gradient -- against the componentwise
precision contract that tests/test_gpu_split_precision.py holds the split-operand entries to and tests/test_gpu_eval_precision.py the
inference entries.

Each case of tests/split_ref.py (GRAD32_CASES) runs through the public route -- the operators of mode_hip.functional for the 3-D, 3 x 3
and spherical families, the autograd Functions for the stride-2 3 x 3 layer, the 1 x 1 layers, the stem and the integer tables -- with
the arithmetic set by the public switch (set_conv_arith('f32'); route 'default': the default switches, for the roles a default training
step itself runs on fp32 kernels).
Asserted per role:
  * the entries that launched, by name (ENTRIES; a recording stand-in for the ctypes handle), and per case the list of judged roles
    (JUDGED): a route that starts to go elsewhere fails the test instead of emptying it;
  * whole-tensor rms and worst slice of u = |got - want| / op(|a|, |b|) (+ |acc| where the entry adds into a tensor that is there), in
    units of 2^-24, both <= T: a third of the mildest emulated mutant of the THREE-PIECE arithmetic on the case's own inputs, computed on
    the host.  The fp32 kernels' products are exact; what T holds them to is their accumulation and every tail, clamp, transpose and
    partial sum of the hand-written reductions.  Exactly zero is demanded where every product is zero (the positions a stride-2
    SCATTER input gradient only zero-fills, the odd rows and columns behind mode_zero_insert2);
  * every weight gradient is computed twice and returns the same bits.
tests/test_split_ref_host.py shows on the CPU, for every one of these roles, that a faithful kernel with an fp32 accumulator stays below
T / 1.5 and that a lost product, a reduction tail that meets zero, a lost K-slice, a lost last pixel segment and a dropped tap, each
confined to one block of output channels, exceed T -- and by which factor the max-abs bounds of tests/test_gpu_kernels.py admit them.

Entries and the cases that reach them:
  mode_conv3d_fwd / _bwd_data / _bwd_weight    conv3d_s1, conv3d_s2 (csrc/conv3d_f32_fwd.hip, conv3d_f32_wgrad.hip; the stride-2 input
                                               gradient is the transposed kernel), conv3d_c1 (Co = 1: csrc/conv3d_c1.hip, all three)
  mode_deconv3d_fwd                            deconv3d forward; its gradients are mode_conv3d_fwd stride 2 on gy and
                                               mode_conv3d_bwd_weight stride 2 with the operands exchanged
  mode_conv2d_fwd / _bwd_data / _bwd_weight    conv2d, dilation 1 and 2 (csrc/conv2d_f32_fwd.hip, conv2d_f32_wgrad.hip)
  mode_sphere_conv_fwd, mode_zero_insert2 +    conv2d_s2: Conv2d3x3S2Function (integer-table forward, both gradients as stride-1
    mode_conv2d_bwd_data / _bwd_weight         gradients of the zero-inserted output gradient)
  mode_conv1x1_fwd / _bwd_data / _bwd_weight   conv1x1, stride 1 and 2 (SCATTER), an odd input height included (csrc/conv1x1.hip)
  mode_conv_stem_fwd / _bwd_weight             conv_stem (csrc/conv_stem.hip)
  mode_sphere_conv_fwd, _bwd_data (atomic      sphere_gen: the gather kernels of csrc/sphere_conv.hip on three general tables (ERP 16 x 32
    scatter), _bwd_data_adj, _bwd_weight,      stride 1 and 2, Cassini 32 x 16 with groups 2), each form behind its public switch (SPHERE_FWD,
    _bwd_weight_win (fp32 window)              SPHERE_BWD_DATA, SPHERE_BWD_DATA_T, SPHERE_BWD_WEIGHT), and through Conv2dTabledFunction on the
                                               integer tables at k = 3 stride 2 and k = 5 stride 3
mode_sphere_conv_bwd_data_adj_list runs only beside the windowed split kernel and is judged with it in tests/test_gpu_split_precision.py;
the stride-2 3-D forward to 128 output channels has no kernel, and the refusal is asserted below (tests/split_ref.py, G32_NO_FORWARD).

MEASURED on an MI355X (one run of this file; T is computed, rms and worst slice are measured; for each family, role (and form), kind of
data the shape with the least room, i.e. the largest worst slice / T, and over how many shapes).  KNOWN is empty: nothing misses T.

family     route   role (form)                            entry                                          data                           T    rms  worst  at the shape (of n), slice
conv3d_s1  f32     forward                                conv3d_fwd                                     unit variance              0.834  0.473  0.507  1x32x32x6x10x40 (3), axis 4 @ 13
conv3d_s1  f32     input gradient                         conv3d_bwd_data                                unit variance              0.768  0.477  0.505  2x20x40x5x7x33 (3), axis 4 @ 19
conv3d_s1  f32     weight gradient                        conv3d_bwd_weight                              unit variance              0.487  0.180  0.190  1x32x32x6x10x40 (3), axis 1 @ 27
conv3d_s1  f32     weight gradient + acc                  conv3d_bwd_weight                              unit variance              0.486  0.180  0.190  1x32x32x6x10x40 (3), axis 1 @ 27
conv3d_s1  f32     forward                                conv3d_fwd                                     six decades along a row    1.239  0.506  0.820  1x32x32x6x10x40 (3), axis 1 @ 6
conv3d_s1  f32     input gradient                         conv3d_bwd_data                                six decades along a row    1.612  0.563  1.162  2x16x20x5x7x33 (3), axis 1 @ 2
conv3d_s1  f32     weight gradient                        conv3d_bwd_weight                              six decades along a row    3.292  1.580  1.745  1x32x32x6x10x40 (3), axis 0 @ 3
conv3d_s1  f32     weight gradient + acc                  conv3d_bwd_weight                              six decades along a row    3.202  1.590  1.746  1x32x32x6x10x40 (3), axis 0 @ 3
conv3d_s1  f32     input gradient                         conv3d_bwd_data                                gradient-sized             0.768  0.475  0.518  2x20x40x5x7x33 (3), axis 4 @ 12
conv3d_s1  f32     weight gradient                        conv3d_bwd_weight                              gradient-sized             0.487  0.181  0.193  1x32x32x6x10x40 (3), axis 0 @ 16
conv3d_s1  f32     weight gradient + acc                  conv3d_bwd_weight                              gradient-sized             0.486  0.181  0.194  1x32x32x6x10x40 (3), axis 1 @ 8
conv3d_s2  f32     forward                                conv3d_fwd                                     unit variance              1.341  0.460  0.517  2x12x24x6x10x36 (1), axis 1 @ 14
conv3d_s2  f32     input gradient                         conv3d_bwd_data                                unit variance              1.599  0.479  0.534  3x64x128x2x4x8 (2), axis 1 @ 2
conv3d_s2  f32     weight gradient                        conv3d_bwd_weight                              unit variance              1.038  0.124  0.137  2x12x24x6x10x36 (2), axis 2 @ 0
conv3d_s2  f32     weight gradient + acc                  conv3d_bwd_weight                              unit variance              1.031  0.127  0.139  2x12x24x6x10x36 (2), axis 2 @ 0
conv3d_s2  f32     forward                                conv3d_fwd                                     six decades along a row    1.975  0.515  0.727  2x12x24x6x10x36 (1), axis 1 @ 7
conv3d_s2  f32     input gradient                         conv3d_bwd_data                                six decades along a row    2.547  0.540  0.657  3x64x128x2x4x8 (2), axis 4 @ 5
conv3d_s2  f32     weight gradient                        conv3d_bwd_weight                              six decades along a row    6.189  0.822  0.882  2x12x24x6x10x36 (2), axis 0 @ 5
conv3d_s2  f32     weight gradient + acc                  conv3d_bwd_weight                              six decades along a row    5.792  0.882  0.950  2x12x24x6x10x36 (2), axis 0 @ 12
conv3d_s2  f32     input gradient                         conv3d_bwd_data                                gradient-sized             1.599  0.470  0.551  3x64x128x2x4x8 (2), axis 1 @ 36
conv3d_s2  f32     weight gradient                        conv3d_bwd_weight                              gradient-sized             1.039  0.123  0.136  2x12x24x6x10x36 (2), axis 2 @ 0
conv3d_s2  f32     weight gradient + acc                  conv3d_bwd_weight                              gradient-sized             1.033  0.126  0.138  2x12x24x6x10x36 (2), axis 0 @ 22
deconv3d   f32     forward                                deconv3d_fwd                                   unit variance              3.001  0.470  0.501  2x24x40x3x5x34 (2), axis 4 @ 14
deconv3d   f32     input gradient                         conv3d_fwd                                     unit variance              0.744  0.475  0.525  2x24x40x3x5x34 (2), axis 1 @ 17
deconv3d   f32     weight gradient                        conv3d_bwd_weight                              unit variance              1.020  0.146  0.164  2x24x40x3x5x34 (2), axis 3 @ 0
deconv3d   f32     weight gradient + acc                  conv3d_bwd_weight                              unit variance              1.013  0.148  0.167  2x24x40x3x5x34 (2), axis 3 @ 0
deconv3d   f32     forward                                deconv3d_fwd                                   six decades along a row    4.153  0.475  0.526  2x24x40x3x5x34 (2), axis 1 @ 12
deconv3d   f32     input gradient                         conv3d_fwd                                     six decades along a row    1.058  0.469  0.609  2x24x40x3x5x34 (2), axis 1 @ 7
deconv3d   f32     weight gradient                        conv3d_bwd_weight                              six decades along a row    6.510  0.881  0.952  2x24x40x3x5x34 (2), axis 0 @ 5
deconv3d   f32     weight gradient + acc                  conv3d_bwd_weight                              six decades along a row    6.223  0.938  0.991  2x24x40x3x5x34 (2), axis 1 @ 15
deconv3d   f32     input gradient                         conv3d_fwd                                     gradient-sized             0.744  0.468  0.509  2x24x40x3x5x34 (2), axis 4 @ 7
deconv3d   f32     weight gradient                        conv3d_bwd_weight                              gradient-sized             1.014  0.143  0.162  2x24x40x3x5x34 (2), axis 2 @ 0
deconv3d   f32     weight gradient + acc                  conv3d_bwd_weight                              gradient-sized             1.007  0.146  0.165  2x24x40x3x5x34 (2), axis 2 @ 0
conv3d_c1  f32     forward                                conv3d_fwd                                     unit variance              0.824  0.122  0.145  2x32x6x12x40 (3), axis 3 @ 0
conv3d_c1  f32     input gradient                         conv3d_bwd_data                                unit variance              4.433  0.467  0.583  2x32x6x12x40 (3), axis 1 @ 3
conv3d_c1  f32     weight gradient                        conv3d_bwd_weight                              unit variance              0.565  0.100  0.109  2x32x6x12x40 (3), axis 3 @ 0
conv3d_c1  f32     weight gradient + acc                  conv3d_bwd_weight                              unit variance              0.563  0.102  0.109  2x32x6x12x40 (3), axis 3 @ 0
conv3d_c1  f32     forward                                conv3d_fwd                                     six decades along a row    1.120  0.155  0.180  2x32x6x12x40 (3), axis 2 @ 5
conv3d_c1  f32     input gradient                         conv3d_bwd_data                                six decades along a row    6.574  0.472  0.571  2x32x6x12x40 (3), axis 1 @ 27
conv3d_c1  f32     weight gradient                        conv3d_bwd_weight                              six decades along a row    3.626  0.858  0.931  2x32x6x12x40 (3), axis 4 @ 2
conv3d_c1  f32     weight gradient + acc                  conv3d_bwd_weight                              six decades along a row    3.497  0.919  1.002  2x32x6x12x40 (3), axis 4 @ 2
conv3d_c1  f32     input gradient                         conv3d_bwd_data                                gradient-sized             4.542  0.465  0.581  2x32x6x12x40 (3), axis 1 @ 3
conv3d_c1  f32     weight gradient                        conv3d_bwd_weight                              gradient-sized             1.130  0.216  0.219  1x20x3x5x33 (3), axis 1 @ 0
conv3d_c1  f32     weight gradient + acc                  conv3d_bwd_weight                              gradient-sized             1.121  0.218  0.223  1x20x3x5x33 (3), axis 1 @ 0
conv2d     f32     forward                                conv2d_fwd                                     unit variance              1.684  0.475  0.535  2x20x40x9x40x1 (3), axis 1 @ 27
conv2d     f32     input gradient                         conv2d_bwd_data                                unit variance              1.191  0.477  0.567  2x20x40x9x40x1 (3), axis 3 @ 12
conv2d     f32     weight gradient                        conv2d_bwd_weight                              unit variance              1.035  0.140  0.152  2x20x40x9x40x1 (3), axis 1 @ 19
conv2d     f32     weight gradient + acc                  conv2d_bwd_weight                              unit variance              1.029  0.144  0.158  2x20x40x9x40x1 (3), axis 1 @ 19
conv2d     f32     forward                                conv2d_fwd                                     six decades along a row    2.403  0.503  0.928  2x20x40x9x40x1 (3), axis 1 @ 36
conv2d     f32     input gradient                         conv2d_bwd_data                                six decades along a row    1.642  0.480  0.735  2x20x40x9x40x1 (3), axis 1 @ 3
conv2d     f32     weight gradient                        conv2d_bwd_weight                              six decades along a row    5.286  0.987  0.987  2x3x5x5x70x2 (3), axis 0 @ 0
conv2d     f32     weight gradient + acc                  conv2d_bwd_weight                              six decades along a row    5.002  1.029  1.029  2x3x5x5x70x2 (3), axis 0 @ 0
conv2d     f32     input gradient                         conv2d_bwd_data                                gradient-sized             1.185  0.471  0.537  2x20x40x9x40x1 (3), axis 3 @ 18
conv2d     f32     weight gradient                        conv2d_bwd_weight                              gradient-sized             0.950  0.146  0.146  2x3x5x5x70x2 (3), axis 0 @ 0
conv2d     f32     weight gradient + acc                  conv2d_bwd_weight                              gradient-sized             0.943  0.149  0.149  2x3x5x5x70x2 (3), axis 0 @ 0
conv2d_s2  f32     forward                                sphere_conv_fwd                                unit variance              1.665  0.471  0.542  1x20x40x10x36 (2), axis 1 @ 18
conv2d_s2  f32     input gradient                         zero_insert2 + conv2d_bwd_data                 unit variance              2.586  0.493  0.551  1x20x40x10x36 (2), axis 1 @ 17
conv2d_s2  f32     weight gradient                        zero_insert2 + conv2d_bwd_weight               unit variance              2.367  0.248  0.277  1x20x40x10x36 (2), axis 0 @ 22
conv2d_s2  f32     weight gradient + acc                  zero_insert2 + conv2d_bwd_weight               unit variance              2.333  0.254  0.288  1x20x40x10x36 (2), axis 0 @ 20
conv2d_s2  f32     forward                                sphere_conv_fwd                                six decades along a row    2.556  0.474  0.575  1x20x40x10x36 (2), axis 1 @ 36
conv2d_s2  f32     input gradient                         zero_insert2 + conv2d_bwd_data                 six decades along a row    3.603  0.472  0.529  1x20x40x10x36 (2), axis 3 @ 4
conv2d_s2  f32     weight gradient                        zero_insert2 + conv2d_bwd_weight               six decades along a row   10.156  0.915  0.987  1x20x40x10x36 (2), axis 1 @ 3
conv2d_s2  f32     weight gradient + acc                  zero_insert2 + conv2d_bwd_weight               six decades along a row    9.195  0.920  1.025  1x20x40x10x36 (2), axis 1 @ 15
conv2d_s2  f32     input gradient                         zero_insert2 + conv2d_bwd_data                 gradient-sized             2.573  0.476  0.538  1x20x40x10x36 (2), axis 3 @ 16
conv2d_s2  f32     weight gradient                        zero_insert2 + conv2d_bwd_weight               gradient-sized             2.314  0.247  0.267  1x20x40x10x36 (2), axis 0 @ 22
conv2d_s2  f32     weight gradient + acc                  zero_insert2 + conv2d_bwd_weight               gradient-sized             3.707  0.431  0.465  2x8x8x2x4 (2), axis 0 @ 4
conv1x1    f32     forward                                conv1x1_fwd                                    unit variance              1.343  0.476  0.576  1x256x128x8x16x1 (5), axis 1 @ 122
conv1x1    f32     input gradient                         conv1x1_bwd_data                               unit variance              1.543  0.472  0.516  2x12x200x6x8x1 (5), axis 3 @ 4
conv1x1    f32     weight gradient                        conv1x1_bwd_weight                             unit variance              1.339  0.247  0.295  2x64x64x16x32x2 (5), axis 1 @ 28
conv1x1    f32     weight gradient + acc                  conv1x1_bwd_weight                             unit variance              1.329  0.247  0.293  2x64x64x16x32x2 (5), axis 1 @ 28
conv1x1    f32     forward                                conv1x1_fwd                                    six decades along a row    1.874  0.468  0.607  1x256x128x8x16x1 (5), axis 1 @ 48
conv1x1    f32     input gradient                         conv1x1_bwd_data                               six decades along a row    2.653  0.467  0.655  1x256x128x8x16x1 (5), axis 1 @ 36
conv1x1    f32     weight gradient                        conv1x1_bwd_weight                             six decades along a row    8.067  0.985  1.090  2x64x64x16x32x2 (5), axis 1 @ 24
conv1x1    f32     weight gradient + acc                  conv1x1_bwd_weight                             six decades along a row    7.311  0.965  1.072  2x64x64x16x32x2 (5), axis 1 @ 36
conv1x1    f32     input gradient                         conv1x1_bwd_data                               gradient-sized             1.555  0.472  0.534  2x12x200x6x8x1 (5), axis 1 @ 9
conv1x1    f32     weight gradient                        conv1x1_bwd_weight                             gradient-sized             1.322  0.243  0.264  2x64x64x16x32x2 (5), axis 1 @ 40
conv1x1    f32     weight gradient + acc                  conv1x1_bwd_weight                             gradient-sized             1.311  0.244  0.266  2x64x64x16x32x2 (5), axis 1 @ 28
conv_stem  f32     forward                                conv_stem_fwd                                  unit variance              1.900  0.470  0.526  2x20x26x70 (2), axis 1 @ 3
conv_stem  f32     weight gradient                        conv_stem_bwd_weight                           unit variance              0.745  0.106  0.115  2x20x26x70 (2), axis 2 @ 0
conv_stem  f32     weight gradient + acc                  conv_stem_bwd_weight                           unit variance              0.742  0.108  0.117  2x20x26x70 (2), axis 2 @ 0
conv_stem  f32     forward                                conv_stem_fwd                                  six decades along a row    3.480  0.998  1.046  1x32x8x8 (2), axis 3 @ 2
conv_stem  f32     weight gradient                        conv_stem_bwd_weight                           six decades along a row    4.724  0.845  0.920  2x20x26x70 (2), axis 0 @ 0
conv_stem  f32     weight gradient + acc                  conv_stem_bwd_weight                           six decades along a row    4.646  0.931  1.032  2x20x26x70 (2), axis 0 @ 0
conv_stem  f32     weight gradient                        conv_stem_bwd_weight                           gradient-sized             0.719  0.109  0.117  2x20x26x70 (2), axis 2 @ 0
conv_stem  f32     weight gradient + acc                  conv_stem_bwd_weight                           gradient-sized             0.716  0.110  0.119  2x20x26x70 (2), axis 2 @ 0
sphere_gen f32     forward (gather)                       sphere_conv_fwd                                unit variance              1.533  0.416  0.485  ERPx16x32x2x16x32x1x2 (3), axis 1 @ 30
sphere_gen f32     input gradient (atomic scatter)        sphere_conv_bwd_data                           unit variance              1.227  0.207  0.366  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 0
sphere_gen f32     input gradient (adjoint gather)        sphere_conv_bwd_data_adj                       unit variance              1.227  0.417  0.628  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 0
sphere_gen f32     input gradient + acc (atomic scatter)  sphere_conv_bwd_data                           unit variance              1.212  0.208  0.371  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 0
sphere_gen f32     input gradient + acc (adjoint gather)  sphere_conv_bwd_data_adj                       unit variance              1.212  0.415  0.617  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 0
sphere_gen f32     weight gradient (gather)               sphere_conv_bwd_weight                         unit variance              0.579  0.114  0.133  Cassinix32x16x2x12x40x2x1 (3), axis 3 @ 1
sphere_gen f32     weight gradient (fp32 window)          sphere_conv_bwd_weight_win                     unit variance              0.579  0.145  0.173  Cassinix32x16x2x12x40x2x1 (2), axis 3 @ 1
sphere_gen f32     weight gradient + acc (gather)         sphere_conv_bwd_weight                         unit variance              0.577  0.116  0.135  Cassinix32x16x2x12x40x2x1 (3), axis 3 @ 1
sphere_gen f32     weight gradient + acc (fp32 window)    sphere_conv_bwd_weight_win                     unit variance              0.577  0.145  0.174  Cassinix32x16x2x12x40x2x1 (2), axis 3 @ 1
sphere_gen f32     forward (gather)                       sphere_conv_fwd                                six decades along a row    3.216  0.809  1.344  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 1
sphere_gen f32     input gradient (atomic scatter)        sphere_conv_bwd_data                           six decades along a row    2.324  0.353  0.571  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 2
sphere_gen f32     input gradient (adjoint gather)        sphere_conv_bwd_data_adj                       six decades along a row    2.324  0.764  1.214  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 2
sphere_gen f32     input gradient + acc (atomic scatter)  sphere_conv_bwd_data                           six decades along a row    2.318  0.353  0.561  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 2
sphere_gen f32     input gradient + acc (adjoint gather)  sphere_conv_bwd_data_adj                       six decades along a row    2.318  0.765  1.216  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 2
sphere_gen f32     weight gradient (gather)               sphere_conv_bwd_weight                         six decades along a row    3.523  0.856  0.886  Cassinix32x16x2x12x40x2x1 (3), axis 1 @ 1
sphere_gen f32     weight gradient (fp32 window)          sphere_conv_bwd_weight_win                     six decades along a row    3.523  1.976  2.211  Cassinix32x16x2x12x40x2x1 (2), axis 3 @ 0
sphere_gen f32     weight gradient + acc (gather)         sphere_conv_bwd_weight                         six decades along a row    3.422  0.928  0.962  Cassinix32x16x2x12x40x2x1 (3), axis 1 @ 1
sphere_gen f32     weight gradient + acc (fp32 window)    sphere_conv_bwd_weight_win                     six decades along a row    3.422  1.943  2.117  Cassinix32x16x2x12x40x2x1 (2), axis 0 @ 5
sphere_gen f32     input gradient (atomic scatter)        sphere_conv_bwd_data                           gradient-sized             1.227  0.207  0.387  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 0
sphere_gen f32     input gradient (adjoint gather)        sphere_conv_bwd_data_adj                       gradient-sized             1.227  0.428  0.674  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 0
sphere_gen f32     input gradient + acc (atomic scatter)  sphere_conv_bwd_data                           gradient-sized             1.211  0.204  0.367  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 0
sphere_gen f32     input gradient + acc (adjoint gather)  sphere_conv_bwd_data_adj                       gradient-sized             1.211  0.427  0.666  ERPx16x32x2x16x32x1x1 (3), axis 2 @ 0
sphere_gen f32     weight gradient (gather)               sphere_conv_bwd_weight                         gradient-sized             0.577  0.114  0.129  Cassinix32x16x2x12x40x2x1 (3), axis 3 @ 1
sphere_gen f32     weight gradient (fp32 window)          sphere_conv_bwd_weight_win                     gradient-sized             0.577  0.148  0.177  Cassinix32x16x2x12x40x2x1 (2), axis 3 @ 1
sphere_gen f32     weight gradient + acc (gather)         sphere_conv_bwd_weight                         gradient-sized             0.587  0.117  0.133  ERPx16x32x2x16x32x1x1 (3), axis 3 @ 1
sphere_gen f32     weight gradient + acc (fp32 window)    sphere_conv_bwd_weight_win                     gradient-sized             0.575  0.148  0.176  Cassinix32x16x2x12x40x2x1 (2), axis 3 @ 1
sphere_gen f32     forward (integer table)                sphere_conv_fwd                                unit variance              2.324  0.477  0.477  tablex5x3x1x6x4x10x13 (2), axis 0 @ 0
sphere_gen f32     input gradient (integer table)         sphere_conv_bwd_data_adj                       unit variance              5.247  0.486  0.486  tablex3x2x1x5x7x9x11 (2), axis 0 @ 0
sphere_gen f32     weight gradient (integer table)        sphere_conv_bwd_weight                         unit variance              3.722  0.465  0.465  tablex3x2x1x5x7x9x11 (2), axis 0 @ 0
sphere_gen f32     weight gradient + acc (integer table)  sphere_conv_bwd_weight                         unit variance              3.614  0.476  0.476  tablex3x2x1x5x7x9x11 (2), axis 0 @ 0
sphere_gen f32     forward (integer table)                sphere_conv_fwd                                six decades along a row    4.652  0.662  0.662  tablex5x3x1x6x4x10x13 (2), axis 0 @ 0
sphere_gen f32     input gradient (integer table)         sphere_conv_bwd_data_adj                       six decades along a row    7.635  0.516  0.545  tablex5x3x1x6x4x10x13 (2), axis 2 @ 4
sphere_gen f32     weight gradient (integer table)        sphere_conv_bwd_weight                         six decades along a row   10.180  0.666  0.733  tablex5x3x1x6x4x10x13 (2), axis 0 @ 2
sphere_gen f32     weight gradient + acc (integer table)  sphere_conv_bwd_weight                         six decades along a row    7.360  0.630  0.656  tablex5x3x1x6x4x10x13 (2), axis 0 @ 2
sphere_gen f32     input gradient (integer table)         sphere_conv_bwd_data_adj                       gradient-sized             5.266  0.476  0.476  tablex3x2x1x5x7x9x11 (2), axis 1 @ 0
sphere_gen f32     weight gradient (integer table)        sphere_conv_bwd_weight                         gradient-sized             3.906  0.456  0.456  tablex3x2x1x5x7x9x11 (2), axis 1 @ 0
sphere_gen f32     weight gradient + acc (integer table)  sphere_conv_bwd_weight                         gradient-sized             3.796  0.455  0.455  tablex3x2x1x5x7x9x11 (2), axis 0 @ 0
conv3d_s1  default input gradient                         conv3d_bwd_data                                unit variance              1.090  0.468  0.496  2x16x20x5x7x33 (1), axis 4 @ 5
conv3d_s1  default input gradient                         conv3d_bwd_data                                six decades along a row    1.609  0.521  0.796  2x16x20x5x7x33 (1), axis 1 @ 12
conv3d_s1  default input gradient                         conv3d_bwd_data                                gradient-sized             1.090  0.466  0.505  2x16x20x5x7x33 (1), axis 4 @ 5
conv2d     default input gradient                         conv2d_bwd_data                                unit variance              1.224  0.467  0.537  2x16x40x7x33x1 (1), axis 1 @ 5
conv2d     default input gradient                         conv2d_bwd_data                                six decades along a row    1.796  0.514  0.707  2x16x40x7x33x1 (1), axis 1 @ 1
conv2d     default input gradient                         conv2d_bwd_data                                gradient-sized             1.224  0.461  0.522  2x16x40x7x33x1 (1), axis 3 @ 26
"""
import pytest
import torch

import cpu_threads
import mode_hip
import split_ref as S
from mode_hip import functional as HF
from test_gpu_size_contracts import recorder  # noqa: F401  (the fixture that records the launching entries by name)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SWITCHES = ('CONV3D_S1_F16', 'CONV2D_F16', 'SPHERE_FWD', 'SPHERE_BWD_WEIGHT', 'SPHERE_BWD_DATA', 'SPHERE_BWD_DATA_T', 'SPHERE_BWD_DATA_SPLIT',
            'SPHERE_BWD_SPLIT_MIN_WG')


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  mode_hip.lib()
  torch.set_num_threads(cpu_threads.usable_cores())


@pytest.fixture
def switches():
  """The route switches of mode_hip.functional, restored after the case."""
  keep = (HF.CONV_ARITH,) + tuple(getattr(HF, n) for n in SWITCHES)
  yield
  HF.set_conv_arith(keep[0])
  for n, v in zip(SWITCHES, keep[1:]):
    setattr(HF, n, v)


def _set_route(case):
  if case.route == 'f32':
    HF.set_conv_arith('f32')
  else:
    assert (HF.CONV_ARITH, HF.CONV3D_S1_F16, HF.CONV2D_F16) == ('bf16x6', True, True)  # the default training step


COMPUTE = ('mode_conv', 'mode_deconv', 'mode_sphere_conv', 'mode_zero_insert2')

# (family, role) -> the entries that must launch, in order.  '+ acc' roles launch what the role without it does.
_C3 = {'forward': ['mode_conv3d_fwd'], 'input gradient': ['mode_conv3d_bwd_data'], 'weight gradient': ['mode_conv3d_bwd_weight']}
_C2 = {'forward': ['mode_conv2d_fwd'], 'input gradient': ['mode_conv2d_bwd_data'], 'weight gradient': ['mode_conv2d_bwd_weight']}
ENTRIES = {
    'conv3d_s1': _C3, 'conv3d_s2': _C3, 'conv3d_c1': _C3,
    'deconv3d': {'forward': ['mode_deconv3d_fwd'], 'input gradient': ['mode_conv3d_fwd'], 'weight gradient': ['mode_conv3d_bwd_weight']},
    'conv2d': _C2,
    'conv2d_s2': {'forward': ['mode_sphere_conv_fwd'], 'input gradient': ['mode_zero_insert2', 'mode_conv2d_bwd_data'],
                  'weight gradient': ['mode_zero_insert2', 'mode_conv2d_bwd_weight']},
    'conv1x1': {'forward': ['mode_conv1x1_fwd'], 'input gradient': ['mode_conv1x1_bwd_data'], 'weight gradient': ['mode_conv1x1_bwd_weight']},
    'conv_stem': {'forward': ['mode_conv_stem_fwd'], 'weight gradient': ['mode_conv_stem_bwd_weight']},
}

# The roles of each case that are judged, written out (the 'gradient-sized' kind has no forward; the stem no input gradient).
ALL = ('forward', 'input gradient', 'weight gradient', 'weight gradient + acc')
JUDGED = {(fam, 'f32'): ALL for fam in ENTRIES}
JUDGED[('sphere_gen', 'f32')] = ('forward', 'input gradient', 'input gradient + acc', 'weight gradient', 'weight gradient + acc')
JUDGED.update({('sphere_gen', 'f32', shape): ALL for shape in S.G32_SPHERE_GEN if shape[0] == 'table'})
JUDGED[('conv_stem', 'f32')] = ('forward', 'weight gradient', 'weight gradient + acc')
JUDGED.update({(fam, 'default', shape): names for fam, shape, names in S.G32_DEFAULT})
JUDGED.update({(fam, 'f32', shape): ALL[1:] for fam, shape in S.G32_NO_FORWARD})


def _judged(case):
  names = JUDGED.get((case.family, case.route, case.shape)) or JUDGED[(case.family, case.route)]
  return [n for n in names if not (n == 'forward' and case.kind == 'gradient-sized')]


def _through_function(apply, role, t):
  """A role of a layer that is reached through its autograd Function: `apply(x, w)` is the layer."""
  d = lambda v: v.to(DEV)
  if role.name == 'forward':
    return lambda: apply(d(role.a), d(role.b))
  if role.name == 'input gradient':
    def run():
      x = d(t['x']).requires_grad_(True)
      y = apply(x, d(role.b))
      return y, lambda: torch.autograd.grad(y, x, d(role.a))[0]
    return run
  def run():  # the weight gradient; with acc: into the parameter's gradient sink (functional.grad_sink), as the data-parallel step does
    w = torch.nn.Parameter(d(t['w']))
    if role.acc is not None:
      w.grad = d(role.acc).clone()
      w._mode_grad_sink = w.grad
    y = apply(d(role.b), w)
    def back():
      if role.acc is None:
        return torch.autograd.grad(y, w, d(role.a))[0]
      y.backward(d(role.a))
      return w.grad
    return y, back
  return run


def _launch(case, role, t):
  """A callable that runs the role on the device.  For the layers behind an autograd Function it returns (y, backward): the forward runs
  first, unrecorded, and `backward()` is what is recorded and judged."""
  fam, name = case.family, role.name
  d = lambda v: v.to(DEV)
  into = (lambda: d(role.acc).clone()) if role.acc is not None else (lambda: None)
  if fam in ('conv3d_s1', 'conv3d_s2', 'conv3d_c1'):
    stride = 2 if fam == 'conv3d_s2' else 1
    if name == 'forward':
      return lambda: HF.conv3d_fwd(d(role.a), d(role.b), stride)
    if name == 'input gradient':
      return lambda: HF.conv3d_bwd_data(d(role.a), d(role.b), tuple(t['x'].shape), stride)
    return lambda: HF.conv3d_bwd_weight(d(role.a), d(role.b), stride, into=into())
  if fam == 'deconv3d':
    if name == 'forward':
      return lambda: HF.deconv3d_fwd(d(role.a), d(role.b))
    if name == 'input gradient':  # (Deconv3dFunction.backward)
      return lambda: HF.conv3d_fwd(d(role.a), d(role.b), 2)
    return lambda: HF.conv3d_bwd_weight(d(role.a), d(role.b), 2, into=into())
  if fam == 'conv2d':
    dil = case.shape[5]
    if name == 'forward':
      return lambda: HF.conv2d_fwd(d(role.a), d(role.b), dil)
    if name == 'input gradient':
      return lambda: HF.conv2d_bwd_data(d(role.a), d(role.b), dil)
    return lambda: HF.conv2d_bwd_weight(d(role.a), d(role.b), dil, into=into())
  if fam == 'conv2d_s2':
    return _through_function(lambda x, w: HF.Conv2d3x3S2Function.apply(x, w), role, t)
  if fam == 'conv1x1':
    s = case.shape[5]
    return _through_function(lambda x, w: HF.Conv1x1Function.apply(x, w, s), role, t)
  assert fam == 'conv_stem'
  return _through_function(lambda x, w: HF.ConvStemFunction.apply(x, w), role, t)


def _sphere_forms(case, role, t):
  """[(label, entries, run)]: every gather-kernel form of csrc/sphere_conv.hip that takes the role, each behind its public switch."""
  d = lambda v: v.to(DEV)
  stride, pad, dil, g = t['geom']
  name = role.name.replace(' + acc', '')
  if case.shape[0] == 'table':  # the integer tables: through Conv2dTabledFunction, on the default switches
    # (the layer takes x, w and gy themselves: the role's operands are the SAMPLED column and gradient, which the kernels form)
    a, b = {'forward': ('x', 'w'), 'input gradient': ('gy', 'w'), 'weight gradient': ('gy', 'x')}[name]
    run = _through_function(lambda x, w: HF.Conv2dTabledFunction.apply(x, w, stride, pad, dil), role._replace(a=t[a], b=t[b]), t)
    H, W = t['x'].shape[2:]
    assert torch.equal(HF.conv2d_table(H, W, t['w'].shape[2], t['w'].shape[3], stride, pad, dil, torch.device(DEV)).cpu(), t['pos'])
    entry = {'forward': 'mode_sphere_conv_fwd', 'input gradient': 'mode_sphere_conv_bwd_data_adj', 'weight gradient': 'mode_sphere_conv_bwd_weight'}[name]
    return [('integer table', [entry], run)]
  pos = d(t['pos'])
  x, w, gy = d(t['x']), d(t['w']), d(t['gy'])
  if name == 'forward':
    def run():
      HF.SPHERE_FWD = 'gather'
      return HF.sphere_conv_fwd(x, pos, w, torch.full(tuple(gy.shape), float('nan'), device=DEV), stride, g)
    return [('gather', ['mode_sphere_conv_fwd'], run)]
  if name == 'input gradient':
    def form(how, transposed):
      def run():
        HF.SPHERE_BWD_DATA, HF.SPHERE_BWD_DATA_T = how, transposed
        gx = d(role.acc).clone() if role.acc is not None else torch.full(tuple(x.shape), float('nan'), device=DEV)
        return HF.sphere_conv_bwd_data(gy, pos, w, gx, stride, g, overwrite=role.acc is None)
      return run
    return [('atomic scatter', ['mode_sphere_conv_bwd_data'], form('scatter', True)),
            ('adjoint gather', ['mode_sphere_conv_bwd_data_adj'], form('gather', False))]
  def form(how):
    def run():
      HF.SPHERE_BWD_WEIGHT = how
      gw = d(role.acc).clone() if role.acc is not None else torch.zeros(tuple(w.shape), device=DEV)
      return HF.sphere_conv_bwd_weight(gy, pos, x, gw, stride, g)
    return run
  out = [('gather', ['mode_sphere_conv_bwd_weight'], form('gather'))]
  if tuple(stride) == (1, 1):  # the fp32 windowed kernel (CONV_ARITH 'f32'), where the geometry is the windowed kernels'
    out.append(('fp32 window', ['mode_sphere_conv_bwd_weight_win'], form('window')))
  return out


def _forms(case, role, t):
  if case.family == 'sphere_gen':
    return _sphere_forms(case, role, t)
  return [('', ENTRIES[case.family][role.name.replace(' + acc', '')], _launch(case, role, t))]


def _run(recorder, run):
  """(result, the compute entries it launched)."""
  del recorder.names[:]
  got = run()
  if isinstance(got, tuple):  # (the forward of a Function ran; its backward is the role)
    del recorder.names[:]
    got = got[1]()
  torch.cuda.synchronize()
  return got.detach(), [n for n in recorder.names if n.startswith(COMPUTE)]


# FINDINGS: roles that miss T through fp32 accumulation alone (a long running sum on non-negative data), kept in and strict as in the
# sibling files -- allowed only where the same entry passes on the same kind of data at a shorter reduction that is a case of its own,
# and for at most one role in ten.  (case id, role, form) -> the measured figures.
KNOWN = {}


@pytest.mark.parametrize('case', S.GRAD32_CASES, ids=S.grad32_case_id)
def test_fp32_training_entry_keeps_the_componentwise_contract(case, switches, recorder):
  _set_route(case)
  roles, tensors = S.grad32_roles(case)
  shape = 'x'.join(str(v) for v in case.shape)
  judged, missed, expected_misses = [], [], []
  for role, ref in S.grad32_references(case, roles):
    judged.append(role.name)
    for label, entries, run in _forms(case, role, tensors):
      tag = (S.grad32_case_id(case), role.name, label)
      got, ran = _run(recorder, run)
      assert ran == entries, (tag, ran)
      if role.name.startswith('weight gradient'):
        again, ran = _run(recorder, run)
        assert ran == entries and torch.equal(got, again), (tag, 'the second call differs', float((got - again).abs().max()))
      whole, worst, _ = S.measure(case, role, ref, got)
      print('GRAD32PREC | %s | %s | %s | %s%s | %s | %s | T %.3f | rms %.3f | worst slice %.3f (axis %d @ %d)' %
            (case.family, shape, case.route, role.name, ' (%s)' % label if label else '', case.kind, ' + '.join(entries), ref.T, whole, worst.rms,
             worst.axis, worst.index))
      ok = whole <= ref.T and worst.rms <= ref.T
      known = KNOWN.get(tag)
      if known is not None:
        assert not ok, 'this role now meets T (%.3f, worst slice %.3f): take it out of KNOWN' % (ref.T, worst.rms)
        expected_misses.append(known)
      elif not ok:
        missed.append((role.name, label, 'T %.3f' % ref.T, 'rms %.3f' % whole, worst))
  assert judged == _judged(case) and judged, (S.grad32_case_id(case), judged, _judged(case))
  assert not missed, (S.grad32_case_id(case), missed)
  if expected_misses:
    pytest.xfail('; '.join(expected_misses))


def test_the_stride_2_forward_with_128_output_channels_is_refused_not_run(switches):
  """S.G32_NO_FORWARD: neither kernel family takes that forward, under either arithmetic -- the operator raises, it computes nothing."""
  (fam, (B, Ci, Co, D, H, W)), = S.G32_NO_FORWARD
  x, w = torch.zeros((B, Ci, D, H, W), device=DEV), torch.zeros((Co, Ci, 3, 3, 3), device=DEV)
  for arith in ('bf16x6', 'f32'):
    HF.set_conv_arith(arith)
    with pytest.raises(RuntimeError, match='more than 64 output channels'):
      HF.conv3d_fwd(x, w, 2)


def test_known_findings_stay_within_one_role_in_ten():
  n = sum(len(_judged(c)) for c in S.GRAD32_CASES)
  assert len(KNOWN) * 10 <= n, (len(KNOWN), n)
