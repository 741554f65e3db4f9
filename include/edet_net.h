/* Network-level C ABI of the MI355X-native EfficientDet path: a whole inference pass / training step behind one call,
 * for a host without a Python interpreter.  Same library (libedet_hip.so), same error convention (0 = ok, otherwise
 * edet_last_error()) as the operator-level ABI of edet_hip.h.
 *
 * What the reference interface is:   efficientdet/tf2/efficientdet_keras.py:790-799  EfficientDetNet.__init__ (model_name,
 *   config) + build            -> edet_create;      :893-915 EfficientDetNet.call(inputs, training) -> edet_forward;
 *   efficientdet/tf2/train_lib.py:606-684 EfficientDetNetTrain.train_step -> edet_train_step;
 *   efficientdet/tf2/anchors.py:117-165 Anchors.__init__/_generate_boxes -> edet_anchors;
 *   efficientdet/tf2/train.py:184-198 (the distribution strategy's gradient all-reduce) -> edet_dp_init.
 *
 * How it works: the launches of a step are a pure function of (config, batch, image size, storage type).  The Python
 * host (automl_amd/plan.py: record_network) runs the step once with a recorder on the operator-level ABI and writes a
 * PLAN: device buffers (sizes, initial contents of the persistent ones: variables, optimizer slots, moving statistics,
 * tables), named handles, and per program the list of edet_* calls with every device pointer as (buffer, offset), the
 * fork / join of the two head chains as event operations, and the place of the gradient exchange.  edet_create loads a
 * plan (hipMalloc + upload + pointer relocation); edet_forward / edet_train_step issue its calls -- eagerly the first
 * time (one-time kernel attribute setup), then, with edet_net_use_graph(net, 1), as ONE captured hipGraph per program.
 * A compiled host therefore needs this header, libedet_hip.so and a plan file -- no interpreter, no torch.
 *
 * Thread safety: one edet_net_t per host thread (the operator-level ABI keeps per-stream deferred-reduction state).  */
#ifndef EDET_NET_H_
#define EDET_NET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct edet_net edet_net_t;

/* Loads a plan: allocates its buffers on the current HIP device, uploads the initial contents, relocates the pointers.
 * A plan is recorded once by the Python engine (automl_amd/plan.py: record_network) per (config, batch, image size,
 * storage type); it fixes the model, the optimizer and the optimizer's constants.  The network starts in the state the
 * plan was recorded from: variables, optimizer slots, moving statistics, iteration count, and the recorded inputs in
 * "images" / the target buffers (zero-filled in a plan recorded with keep_inputs=False: write them before the first
 * pass).  What changes afterwards is reached by name through the variable functions and the state files below.  A plan
 * whose variable table does not fit its buffers is refused.  */
int edet_create(const char* plan_path, edet_net_t** net_out);
int edet_destroy(edet_net_t* net);

/* Named device buffers of the network: "images" [B,H,W,3] in the storage type; "cls_outputs_<L>" / "box_outputs_<L>"
 * [B,h,w,ld] per pyramid level (the first `channels` elements of a pixel are the logits; properties
 * "<name>.channels/.ld/.height/.width/.elem_bytes"); training: "cls_targets_<L>" int32 [B,h,w,A], "box_targets_<L>" fp32
 * [B,h,w,4A], "mean_num_positives" fp32 [B]; state: "params", "ema", "velocity" (flat fp32 arenas; Adam plans: "velocity" is the first
 * moment, "adam_v" the second), "bn_state" (moving statistics), "loss_sums" fp32[4] (class, box, L2, -: sums of the last step), "hyper" fp32[4]; "drop_mask:<block>"
 * fp32 [B,C] stochastic-depth scales floor(p + u) / p that the host refreshes per step (utils.drop_connect).  */
int edet_net_buffer(edet_net_t* net, const char* name, void** device_ptr, size_t* bytes);
int edet_net_num_buffers(edet_net_t* net);
const char* edet_net_buffer_name(edet_net_t* net, int index);
/* Integer properties: "batch", "height", "width", "min_level", "max_level", "num_classes", "num_anchors",
 * "storage_elem_bytes", "num_train_elems", "<buffer>.channels" ...  */
int edet_net_property(edet_net_t* net, const char* name, int64_t* value);
/* 1 if the plan holds the program ("forward", "train_step"), else 0 */
int edet_net_has_program(edet_net_t* net, const char* program);

/* Synchronous copies between host memory and device buffers (hipMemcpy on the library's HIP runtime), for hosts that do
 * not link the HIP runtime themselves; they wait for the device first.  */
int edet_copy_to_host(void* host, const void* device, size_t bytes);
int edet_copy_to_device(void* device, const void* host, size_t bytes);

/* 1: programs are captured into a hipGraph at their second run and replayed afterwards; 0 (default): eager launches */
int edet_net_use_graph(edet_net_t* net, int on);

/* Inference pass over the contents of "images" (EfficientDetNet.call(inputs, training=False)): fills the
 * "cls_outputs_<L>" / "box_outputs_<L>" buffers.  stream: a hipStream_t (NULL = the default stream).  */
int edet_forward(edet_net_t* net, void* stream);

/* Detection on raw images (efficientdet_keras.EfficientDetModel.call, tf2/efficientdet_keras.py:920-1000, with the reference's
 * defaults pre_mode='infer', post_mode='global'): "raw_images" uint8 [B, raw_height, raw_width, 3] -> normalise / resize /
 * pad (:920-951) -> the network -> pre_nms + global NMS + clip + rescale to raw pixels (tf2/postprocess.py:375-406) ->
 * "detections.boxes" fp32 [B, M, 4] (ymin, xmin, ymax, xmax), "detections.scores" fp32 [B, M], "detections.classes" fp32
 * [B, M] (1-based), "detections.valid_len" int32 [B]; M = property "max_output_size".  Plans recorded with
 * record_network(..., detect_raw_hw=(H, W)) hold the program.  */
int edet_detect(edet_net_t* net, void* stream);

/* One training step over "images" and the target buffers (EfficientDetNetTrain.train_step: forward with batch
 * statistics, focal + Huber loss, backward, L2, per-tensor and global-norm clip, [gradient exchange], the update + EMA).
 * The optimizer is the plan's (property "optimizer": 0 = SGD with momentum, 1 = Adam; train_lib.py:176-199; 2 = Lion,
 * lion/lion_tf2.py, with the properties "lion_beta1_bits" / "lion_beta2_bits" / "lion_wd_bits": the doubles' bit patterns
 * of the constants the recorded update launch carries.  Lion has no bias correction: learning_rate reaches its update
 * kernel as it is, as for SGD).
 * learning_rate / ema_decay are this step's RAW values of the schedule (train_lib.py:37-173, :193-197; ema_decay 0 = the
 * plan was recorded without a moving average).  Adam plans: the runtime forms tf.keras Adam's bias-corrected rate itself,
 * alpha = learning_rate * sqrt(1 - beta2^t) / (1 - beta1^t) with t = iterations + 1, in double arithmetic, rounded to
 * float, from the betas the plan holds -- exactly what the Python engine hands its update kernel.  Every step that
 * returns 0 advances the iteration count by one.  An Adam plan written before plans carried the "optimizer" property
 * replays as it always did: learning_rate goes to the update kernel as it is, so the caller passes alpha.  */
int edet_train_step(edet_net_t* net, float learning_rate, float ema_decay, void* stream);

/* ---- variables by name --------------------------------------------------------------------------------------------------
 * The plan's variable table: one entry per variable of the model, in the creation order of the Python host's arena, under
 * the reference's names ("class_net/class-predict/bias", "efficientnet-b0/stem/conv2d/kernel", ...), shapes in the
 * reference's layouts.  Values are fp32.  A trainable variable has the slots VALUE, EMA (the moving-average shadow),
 * MOMENTUM (SGD: the momentum accumulator; Adam: the first moment; Lion: its one slot m) and -- in Adam plans only, so
 * refused for SGD and Lion -- ADAM_V (the second moment); a BatchNorm moving statistic has VALUE only.  Every function refuses a plan recorded without the table.  */
enum { EDET_SLOT_VALUE = 0, EDET_SLOT_EMA = 1, EDET_SLOT_MOMENTUM = 2, EDET_SLOT_ADAM_V = 3 };
typedef struct {
  const char* name;      /* owned by the network, valid until edet_destroy */
  int32_t rank;          /* 0..4 */
  int32_t trainable;
  int64_t dims[4];
  int64_t count;         /* elements = product of dims (1 for rank 0) */
} edet_var_info;
int edet_net_num_variables(edet_net_t* net, int64_t* count);
int edet_net_variable_info(edet_net_t* net, int64_t index, edet_var_info* out);
int edet_net_find_variable(edet_net_t* net, const char* name, int64_t* index);
/* Synchronous, like edet_copy_to_host / _to_device: they wait for the device first.  capacity / count in elements; get
 * wants capacity >= the variable's count, set wants count == it.  Refused, with the variable's name in the message: an
 * unknown name, a wrong count, a slot the variable does not have.  Setting VALUE of a trainable variable while the
 * iteration count is 0 also seeds its EMA shadow (the average starts from the variable, as on the Python host).  */
int edet_get_variable(edet_net_t* net, const char* name, int slot, float* host, int64_t capacity);
int edet_set_variable(edet_net_t* net, const char* name, int slot, const float* host, int64_t count);
/* Optimizer steps applied to the variables: starts at the plan's "iterations" property (0 without it), +1 per successful
 * edet_train_step.  It drives Adam's bias correction; a host's learning-rate schedule reads it.  */
int edet_net_get_iterations(edet_net_t* net, int64_t* iterations);
int edet_net_set_iterations(edet_net_t* net, int64_t iterations);

/* State files: everything a training run needs to resume -- every variable's VALUE, every slot that exists, and the
 * iteration count.  Little endian:
 *   'EDETSTAT'  u32 version (1)  u32 nrecords  i64 iterations
 *   nrecords x { u16 len, name,  u8 slot (EDET_SLOT_*),  u8 rank,  rank x u64 dim,  u64 count,  count x f32 }
 * edet_net_load_state restores by name.  It refuses -- and changes nothing -- when the file names a variable or slot the
 * plan does not have, a record's element count differs from the variable's, a record comes twice, or a variable / slot
 * of the plan is missing from the file.  automl_amd/plan.py read_state / write_state are the same format in numpy: the
 * bridge to the Python host and, through util_keras.save_ckpt / restore_ckpt, to the reference's checkpoints.  */
int edet_net_save_state(edet_net_t* net, const char* path);
int edet_net_load_state(edet_net_t* net, const char* path);

/* Data parallelism (one process per GPU): `fn` is called where the reference's optimizer all-reduces the clipped
 * gradients (train_lib.py:675-683), with the flat fp32 gradient arena, to be summed IN PLACE over the replicas on
 * `stream` (e.g. ncclAllReduce(buf, buf, count, ncclFloat, ncclSum, comm, stream) -- RCCL captures into the step's
 * graph).  fn = NULL: single replica (the default).  */
typedef int (*edet_allreduce_fn)(void* ctx, float* buf, size_t count, void* stream);
int edet_dp_init(edet_net_t* net, edet_allreduce_fn fn, void* ctx);

/* Anchor boxes of tf2/anchors.py Anchors (float64 arithmetic, cast to float32; level-major, then y, x, then
 * a = octave * num_aspects + aspect): boxes_out [count][4] = (ymin, xmin, ymax, xmax) on the HOST.  aspect_ratios: the
 * scalar form (w/h ratio).  boxes_out may be NULL (count only); capacity in boxes.  */
int edet_anchors(int min_level, int max_level, int num_scales, const double* aspect_ratios, int num_aspects,
                 double anchor_scale, int image_height, int image_width, float* boxes_out, int64_t capacity,
                 int64_t* count);

#ifdef __cplusplus
}
#endif
#endif  /* EDET_NET_H_ */
