"""numpy restatement of AutoAugment v0 as automl_amd/autoaugment.py runs it on the RandAugment kernels
(efficientnetv2/autoaugment.py:527-660) -- TEST INFRASTRUCTURE.  The operations are tests/randaug_ref.py's; this file adds the
policy walk: per image the sub-policy, per position floor(float32(u) + float32(prob)) >= 1 as the apply rule (:562-563), the
table's own level through level_to_arg with translate_const 250 and cutout_const 100 (:658), the random negation of the five
signed operations.  It holds no table: the caller passes one (the fixture's, read from the reference)."""
import numpy as np

from tests import randaug_ref as rr

TRANSLATE_CONST, CUTOUT_CONST = 250, 100


def table_of(golden, key):
  """The policy `key` ('v0' / 'test') as tests/golden/reference_autoaug.npz stores the reference's."""
  names, probs, levels = (golden['policy/%s/%s' % (key, part)] for part in ('names', 'probs', 'levels'))
  return [[(str(n), float(p), float(lv) if float(lv) != int(lv) else int(lv)) for n, p, lv in zip(*row)]
          for row in zip(names, probs, levels)]


def applied(u, prob):
  return bool(np.floor(np.float32(u) + np.float32(prob)) >= 1)


def apply_entry(img, name, level, sign):
  args = rr.level_to_arg(name, float(level), TRANSLATE_CONST, CUTOUT_CONST)
  assert name != 'Cutout'      # (its centre draws have no place in autoaug_draws; no policy here holds it)
  if name in rr.SIGNED:
    args = (float(sign) * args[0],)
  return rr.FUNCS[name](img, *args)


def autoaugment_image(img, table, sub, apply_u, sign):
  out = np.array(img, dtype=np.uint8, copy=True)
  for k, (name, prob, level) in enumerate(table[int(sub)]):
    if applied(apply_u[k], prob):
      out = apply_entry(out, name, level, sign[k])
  return out


def autoaugment(images, draws, table):
  """A batch [B, H, W, 3] under draws = (sub [B], apply_u [P, B], sign [P, B]) (autoaugment.autoaug_draws)."""
  sub, apply_u, sign = (np.asarray(d) for d in draws)
  out = np.array(images, dtype=np.uint8, copy=True)
  for i in range(out.shape[0]):
    out[i] = autoaugment_image(out[i], table, sub[i], apply_u[:, i], sign[:, i])
  return out
